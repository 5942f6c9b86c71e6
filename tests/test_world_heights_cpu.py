"""CPU (no GPU needed): the rules behind cvx_world_read_heights / cvx_world_write_heights (cpuvox_amd/csrc/cvx_heights.h), compiled for the host
through tests/heights_rules.cpp, against the independent model of tests/heightsmodel.py (the write expanded into dense arrays and handed to
tests/densemodel.py, the read an argmax over the volume).

- Column mode: thousands of random columns in small worlds (records with 1..3 runs and listed columns, both colour layouts, foreign encodings)
  under random writes (the four ops, sideArgb on and off, thickness 0 / 1 / 2 / 7, WALLED on and off, footprints and windows that stick out),
  against the model re-encoded with tests/pyworld.py's final_column: runs, colours, worldMin / worldMax and the over-limit rejections must match
  exactly.  The program also runs cvxb::DenseColumn on its own expansion of every write and fails when the two rules differ in a word.
- Named column cases; each asserts from the model that it has the property it is named for.
- Read mode: cvxb::HeightsTop over boxes inside, across and outside the world against the model.
- The calls without a context / world, and the wrappers' array checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import heightsmodel
import ruleslib
from cpuvox_amd import gpu
from test_world_brush_cpu import _pick_world
from test_world_dense_cpu import FILL, CARVE, PAINT, REPLACE, _builder_column, _compare, _model_columns, _random_world, read_boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"fill": FILL, "carve": CARVE, "paint": PAINT, "replace": REPLACE}
WALLED = gpu.HEIGHTS_WALLED
TOP, SIDE = 0xFFAA5500, 0xFF0055AA  # the colours of the named cases


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("heights_rules", tmp_path_factory.mktemp("heights"))


# A write is (box_min, y1, heights, argb, side, thickness, flags, op): the footprint is heights.shape at (box_min.x, box_min.z), the window
# [box_min.y, y1).

def write_box(write):
    at, y1, heights = write[0], write[1], write[2]
    return tuple(int(v) for v in at), (int(at[0]) + heights.shape[0], int(y1), int(at[2]) + heights.shape[1])


def _write_words(write):
    """One write as tests/heights_rules.cpp reads it."""
    at, y1, heights, argb, side, thickness, flags, op = write
    words = [np.array(list(at) + [heights.shape[0], y1 - at[1], heights.shape[1], op, thickness, flags, int(argb is not None), int(side is not None)],
                      dtype=np.int64).astype(np.int32), np.ascontiguousarray(heights, dtype=np.int32).ravel()]
    for colours in (argb, side):
        if colours is not None:
            words.append(np.ascontiguousarray(colours, dtype=np.uint32).ravel().view(np.int32))
    return np.concatenate(words)


def model_columns(solid, colour, write):
    """Per column (x-major): (over_limit, runs words, colours, worldMin, worldMax) of the model's result re-encoded by the builder's rule."""
    _, _, heights, argb, side, thickness, flags, op = write
    box = write_box(write)
    argb3, mask3 = heightsmodel.expand(box, heights, argb, side, thickness, flags)
    assert mask3.shape == (heights.shape[0], heights.shape[1], box[1][1] - box[0][1])
    return _model_columns(solid, colour, box[0], argb3, mask3, op)


def _run_columns(rules, tmp_path, cases):
    """cases: (dim_y, gx, gz, stride, [(colorsBase, runs, colours)] x-major, write) -> per case, per column (over, runs, colours, wmin, wmax)."""
    parts = []
    for dim_y, gx, gz, stride, columns, write in cases:
        parts += [ruleslib.world_words(dim_y, gx, gz, stride, columns), _write_words(write)]
    out = ruleslib.run_cases(rules, "columns", tmp_path, *parts)
    results, at = [], 0
    for dim_y, gx, gz, *_ in cases:
        per, at = ruleslib.edited_columns(out, at, gx * gz)
        results.append(per)
    assert at == len(out)
    return results


def _compare_writes(results, models, cases):
    """tests/test_world_dense_cpu.py's comparison; its message reads a dense write's fields."""
    _compare(results, models, [c[:5] + ((c[5][0], None, None, c[5][7]),) for c in cases])


def random_heights(rng, shape, y0, y1, op, carve_without_colours=False):
    """(heights, argb, side or None): heights from three below the window to three above it, colour words of which some are 0."""
    heights = rng.integers(y0 - 3, y1 + 4, size=shape).astype(np.int32)
    argb = rng.integers(0, 2**32, size=shape, dtype=np.uint64).astype(np.uint32)
    argb[rng.random(shape) < 0.1] = 0
    side = rng.integers(0, 2**32, size=shape, dtype=np.uint64).astype(np.uint32) if rng.random() < 0.5 else None
    if op == CARVE and carve_without_colours:
        argb = side = None
    return heights, argb, side


# ---- column mode -------------------------------------------------------------------------------------------------------------------------------

def test_heights_column_rule_matches_the_model(rules, tmp_path):
    rng = np.random.default_rng(4051)
    cases, models = [], []
    columns_total = listed_like = sticking = sided = walled = clamped = 0
    ops, thick = [0, 0, 0, 0], {0: 0, 1: 0, 2: 0, 7: 0}
    for _ in range(900):
        dim_y = int(rng.choice([8, 16, 63, 64, 65, 130, 256]))
        gx, gz = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        stride = int(rng.choice([1, 32]))
        solid, colour, columns, listed = _random_world(rng, gx, dim_y, gz)
        listed_like += listed
        at = [int(rng.integers(-2, gx)), int(rng.integers(-3, dim_y)), int(rng.integers(-2, gz))]
        shape = (int(rng.integers(1, gx + 3)), int(rng.integers(1, gz + 3)))
        y1 = at[1] + int(rng.integers(1, dim_y + 6))
        op = int(rng.integers(0, 4))
        heights, argb, side = random_heights(rng, shape, at[1], y1, op, carve_without_colours=rng.random() < 0.5)
        thickness, flags = int(rng.choice([0, 1, 2, 7])), int(rng.integers(0, 2)) * WALLED
        write = (at, y1, heights, argb, side, thickness, flags, op)
        ops[op] += 1
        thick[thickness] += 1
        sided += side is not None
        walled += flags != 0
        clamped += bool((heights < at[1]).any() or (heights > y1).any())
        sticking += at[1] < 0 or y1 > dim_y
        cases.append((dim_y, gx, gz, stride, columns, write))
        models.append(model_columns(solid, colour, write))
        columns_total += gx * gz
    results = _run_columns(rules, tmp_path, cases)
    _compare_writes(results, models, cases)
    assert columns_total > 3000 and listed_like > 100 and sticking > 100 and sided > 300 and walled > 300 and clamped > 300 and min(ops) > 150 \
        and min(thick.values()) > 150, (columns_total, listed_like, sticking, sided, walled, clamped, ops, thick)


def column_cases(dim_y):
    """Named single-column cases (the GPU test uses them too): name -> (arena spans [lo, hi) of the column, (dx, dz) of the footprint's corner
    relative to it, heights (X, Z), y0, y1, thickness, flags, op).  Every case writes TOP at the top voxel and SIDE below it."""
    one = lambda h: np.array([[h]], dtype=np.int32)  # noqa: E731
    cases = {
        # the window strictly inside one arena run: carved out, the run splits in two
        "window inside a run": ([(4, dim_y - 4)], (0, 0), one(20), 10, 20, 0, 0, CARVE),
        # b exactly on an arena run's top: the runs merge and their colours concatenate
        "b on a run's top": ([(2, 10)], (0, 0), one(20), 0, 30, 10, 0, FILL),
        # H exactly on an arena run's bottom
        "H on a run's bottom": ([(20, 30)], (0, 0), one(20), 5, 40, 5, 0, FILL),
        # b on a run's bottom and H on its top: the run is repainted whole
        "b and H on a run's ends": ([(10, 20)], (0, 0), one(20), 3, 40, 10, 0, PAINT),
        "H == y0": ([(2, 30)], (0, 0), one(10), 10, 20, 0, 0, REPLACE),
        "H == y1": ([(0, 5)], (0, 0), one(20), 10, 20, 0, 0, REPLACE),
        "height below y0": ([(2, 30)], (0, 0), one(-7), 10, 20, 0, 0, REPLACE),
        "height above y1": ([(0, 5)], (0, 0), one(dim_y + 9), 10, 20, 0, 0, REPLACE),
        # the window sticks out below 0 and above dimY; the top voxel lies outside the world
        "window beyond both ends": ([(3, 9)], (0, 0), one(dim_y + 3), -5, dim_y + 7, 0, 0, REPLACE),
        "ends empty": ([(3, 9)], (0, 0), one(0), 0, dim_y, 0, 0, REPLACE),
        # more than three solid runs: a listed record
        "listed": ([(0, 3), (6, 9), (12, 15), (18, 21)], (0, 0), one(32), 0, 40, 2, 0, FILL),
        # a 1 x 1 footprint under WALLED: every neighbour is y0, the crust goes down to the window's bottom
        "1 x 1 walled": ([(0, 2)], (0, 0), one(30), 5, 40, 3, WALLED, REPLACE),
        "1 x 1": ([(0, 2)], (0, 0), one(30), 5, 40, 3, 0, REPLACE),
    }
    for name, (nx, nz) in (("-x", (0, 1)), ("+x", (2, 1)), ("-z", (1, 0)), ("+z", (1, 2))):
        heights = np.full((3, 3), 40, dtype=np.int32)
        heights[nx, nz] = 10  # a cliff of 30, taller than the thickness, towards this neighbour
        cases[f"cliff towards {name}"] = ([(0, 2)], (-1, -1), heights, 0, 44, 2, 0, REPLACE)
    return cases


def column_case_write(case, column=(0, 0)):
    """The write of one of column_cases with the case's column at `column` of the world."""
    _, (dx, dz), heights, y0, y1, thickness, flags, op = case
    argb = np.full(heights.shape, TOP, dtype=np.uint32)
    side = np.full(heights.shape, SIDE, dtype=np.uint32)
    return ((column[0] + dx, y0, column[1] + dz), y1, heights, argb, side, thickness, flags, op)


def arena_colours(dim_y):
    """The colour word a solid voxel of a case's arena column has at height y."""
    return (0xFF000000 | (np.arange(dim_y, dtype=np.uint32) * 40503 & 0xFFFFFF)).astype(np.uint32)


def column_case_arena(dim_y, case):
    """(solid, colour) of the 1 x dim_y x 1 world a case's column is."""
    solid = np.zeros((1, dim_y, 1), dtype=bool)
    for lo, hi in case[0]:
        solid[0, lo:hi, 0] = True
    return solid, np.where(solid, arena_colours(dim_y)[None, :, None], 0).astype(np.uint32)


def boundaries(column):
    """The heights y at which a column (bool over y) changes between y - 1 and y."""
    return set((np.nonzero(column[1:] != column[:-1])[0] + 1).tolist())


def assert_case_properties(dim_y, after):
    """after: name -> (solid, colour) columns over y of the model's result.  Every case has the property it is named for."""
    before_colour = arena_colours(dim_y)
    s, c = after["window inside a run"]
    assert boundaries(s) == {4, 10, 20, dim_y - 4}, "two runs where there was one"
    s, c = after["b on a run's top"]
    assert boundaries(s) == {2, 20} and c[19] == TOP and (c[10:19] == SIDE).all() and (c[2:10] == before_colour[2:10]).all(), "one run, three kinds of colours"
    s, c = after["H on a run's bottom"]
    assert boundaries(s) == {15, 30} and c[19] == TOP and (c[15:19] == SIDE).all() and (c[20:30] == before_colour[20:30]).all()
    s, c = after["b and H on a run's ends"]
    assert boundaries(s) == {10, 20} and c[19] == TOP and (c[10:19] == SIDE).all()
    s, c = after["H == y0"]
    assert boundaries(s) == {2, 10, 20, 30} and not s[10:20].any(), "the window is empty"
    assert all((after["height below y0"][k] == after["H == y0"][k]).all() for k in (0, 1)), "clamped to y0"
    s, c = after["H == y1"]
    assert boundaries(s) == {5, 10, 20} and c[19] == TOP
    assert all((after["height above y1"][k] == after["H == y1"][k]).all() for k in (0, 1)), "clamped to y1"
    s, c = after["window beyond both ends"]
    assert s.all() and (c == SIDE).all(), "solid from 0 to dimY, the top voxel outside the world"
    assert not after["ends empty"][0].any()
    s, c = after["listed"]
    assert len(boundaries(s)) == 9 and s[30:32].all() and not s[29], "five solid runs"
    s, c = after["1 x 1 walled"]
    assert boundaries(s) == {2, 5, 30} and c[29] == TOP and (c[5:29] == SIDE).all(), "a wall down to y0"
    assert boundaries(after["1 x 1"][0]) == {2, 27, 30}, "a crust of three"
    for name in ("-x", "+x", "-z", "+z"):
        s, c = after[f"cliff towards {name}"]
        assert boundaries(s) == {8, 40} and c[39] == TOP and (c[8:39] == SIDE).all(), f"the cliff towards {name} is closed down to two below the neighbour"


@pytest.mark.parametrize("dim_y", [48, 64, 200])
def test_named_column_cases(rules, tmp_path, dim_y):
    cases, models, after = [], [], {}
    named = column_cases(dim_y)
    for name, case in named.items():
        solid, colour = column_case_arena(dim_y, case)
        write = column_case_write(case)
        runs, colours = _builder_column(solid, colour)
        cases.append((dim_y, 1, 1, 1, [(32, runs, colours)], write))
        models.append(model_columns(solid, colour, write))
        s, c = heightsmodel.write(solid, colour, write_box(write), *write[2:])
        after[name] = (s[0, :, 0], c[0, :, 0])
    assert_case_properties(dim_y, after)
    by_name = dict(zip(named, models))
    assert by_name["ends empty"][0] == (False, [], [], 0, 0)
    assert sum(1 for w in by_name["listed"][0][1] if w & 0xFFFF != 0xFFFF) == 5
    results = _run_columns(rules, tmp_path, cases)
    _compare_writes(results, models, cases)


def test_heights_column_rule_rejects_what_the_format_cannot_hold(rules, tmp_path):
    """A run longer than 32767 voxels, a colour index above 32767 and more than 65535 runs, each made by the write together with what the arena
    holds, are over the limit; columns just inside the limits are not.  The tall columns are synthetic, as in tests/test_world_dense_cpu.py."""
    def arena(height, *spans, alternating=None):
        s = np.zeros((1, height, 1), dtype=bool)
        for lo, hi in spans:
            s[0, lo:hi, 0] = True
        if alternating is not None:  # every other voxel from the first to the last of the pair
            s[0, alternating[0]:alternating[1] + 1:2, 0] = True
        c = np.where(s, (0xFF000000 | (np.arange(height, dtype=np.uint32) & 0xFFFFFF))[None, :, None], 0).astype(np.uint32)
        return s, c

    def write(y0, y1, h, thickness=0, op=FILL):
        return ((0, y0, 0), y1, np.array([[h]], dtype=np.int32), np.array([[TOP]], dtype=np.uint32), None, thickness, 0, op)

    specs = [
        (arena(50000, (0, 1)), write(1, 40000, 40000), True),                        # thickness 0 over a tall window: one run of 40000
        (arena(50000, (0, 1)), write(1, 40000, 32767), False),                       # [0, 32767): 32767, fine
        (arena(50000, (0, 1)), write(1, 40000, 32768), True),                        # 32768
        (arena(50000, (0, 10), (30000, 50000)), write(12, 20000, 12 + 12768), True),   # 20000 + 12768 colours above the lowest run: index 32768
        (arena(50000, (0, 10), (30000, 50000)), write(12, 20000, 12 + 12767), False),  # index 32767: fine
        (arena(65536, alternating=(0, 65532)), write(65534, 65536, 65535), True),    # 65534 runs and two more, the last colour index 32767
        (arena(65536, alternating=(2, 65532)), write(65534, 65536, 65535), False),   # 65533 runs and two more: 65535
    ]
    cases, models = [], []
    for (solid, colour), w, _ in specs:
        runs, colours = _builder_column(solid, colour)
        cases.append((solid.shape[1], 1, 1, 1, [(32, runs, colours)], w))
        models.append(model_columns(solid, colour, w))
    want = [over for _, _, over in specs]
    assert [m[0][0] for m in models] == want
    assert len(models[6][0][1]) == 65535 and max(w >> 16 for w in models[1][0][1]) == 32767 and max(w & 0xFFFF for w in models[4][0][1] if w & 0xFFFF != 0xFFFF) == 32767
    results = _run_columns(rules, tmp_path, cases)
    assert [r[0][0] for r in results] == want
    _compare_writes(results, models, cases)


# ---- read mode ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 256, 16), True, 3)])
def test_read_rule_matches_the_model(rules, tmp_path, dims, sparse, seed):
    solid, colour, ws = _pick_world(np.random.default_rng(seed), dims, sparse)
    try:
        info = ws.info(0)
        blob, out = tmp_path / "world.bin", tmp_path / "read.bin"
        blob.write_bytes(ws.storage(0).tobytes())
        layered = 0
        for name, (lo, hi) in read_boxes(dims).items():
            size = [hi[i] - lo[i] for i in range(3)]
            subprocess.check_call([rules, "read", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), *[str(v) for v in lo],
                                   *[str(v) for v in size], str(out)])
            n = size[0] * size[2]
            raw = np.frombuffer(out.read_bytes(), dtype=np.uint32)
            assert raw.size == 3 * n
            heights, argb, bottoms = raw[:n].view(np.int32).reshape(size[0], size[2]), raw[n:2 * n].reshape(size[0], size[2]), raw[2 * n:].view(np.int32).reshape(size[0], size[2])
            want_h, want_a, want_b = heightsmodel.read(solid, colour, (lo, hi))
            if name == "outside":
                assert (want_h == lo[1]).all() and not want_a.any() and (want_b == lo[1]).all()
            elif name in ("whole", "sticks out"):
                assert (want_h > lo[1]).any() and (want_h == lo[1]).any() == (name == "sticks out" or sparse), f"{name}: columns with and without ground"
            layered += int(((want_b > max(lo[1], 0)) & (want_h > lo[1])).sum())
            assert (heights == want_h).all() and (argb == want_a).all() and (bottoms == want_b).all(), name
        assert layered > 50, "top layers that end above the window's bottom"
    finally:
        ws.close()


# ---- entry points -------------------------------------------------------------------------------------------------------------------------------

def test_calls_fail_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2)
    h, argb, b = (C.c_int32 * 4)(), (C.c_uint32 * 4)(), (C.c_int32 * 4)()
    assert L.cvx_world_read_heights(None, lo, hi, h, argb, b, None) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    assert L.cvx_world_read_heights_device(None, lo, hi, h, argb, b, None) == -1
    assert L.cvx_world_write_heights(None, lo, hi, h, argb, None, 1, 0, REPLACE, 0, None) == -1
    assert L.cvx_world_write_heights_device(None, lo, hi, h, argb, None, 1, 0, REPLACE, 0, None) == -1
    # a context without a device or world (tests/heights_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 31 + [-3] * 5, codes
    header = open(os.path.join(ROOT, "include", "cpuvox_gpu_heights.h")).read()
    for name in ("cvx_world_read_heights", "cvx_world_read_heights_device", "cvx_world_write_heights", "cvx_world_write_heights_device"):
        assert name in gpu.HEIGHTS_EXPORTS and re.search(r"\bint " + name + r"\(", header)
    assert re.search(r"#define CVX_HEIGHTS_WALLED\s+1\b", header) and WALLED == 1 == heightsmodel.WALLED
    handle = C.c_void_p()
    if L.cvx_create(0, C.byref(handle)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_read_heights(handle, lo, hi, h, argb, b, None) == -3
            assert L.cvx_world_write_heights(handle, lo, hi, h, argb, None, 1, 0, REPLACE, 0, None) == -3
        finally:
            L.cvx_destroy(handle)


def test_python_wrappers_check_their_arrays():
    ctx = object.__new__(gpu.Context)
    heights = np.zeros((2, 3), dtype=np.int32)
    with pytest.raises(ValueError, match="one shape"):
        gpu.Context.write_heights(ctx, (0, 0, 0), 8, heights, np.zeros((3, 2), dtype=np.uint32))
    with pytest.raises(ValueError, match="one shape"):
        gpu.Context.write_heights(ctx, (0, 0, 0), 8, heights, np.zeros((2, 3), dtype=np.uint32), np.zeros((2, 4), dtype=np.uint32))
    with pytest.raises(ValueError, match="integer array of shape"):
        gpu.Context.write_heights(ctx, (0, 0, 0), 8, np.zeros((2, 3, 1), dtype=np.int32), None)
    with pytest.raises(ValueError, match="integer array of shape"):
        gpu.Context.write_heights(ctx, (0, 0, 0), 8, np.zeros((2, 3), dtype=np.float32), None)
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.write_heights(ctx, (0, 0), 8, heights, np.zeros((2, 3), dtype=np.uint32))
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.read_heights_device(ctx, (0, 0), (1, 1, 1), 0)
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.write_heights_device(ctx, (0, 0, 0), (1, 1), 0, 0)
