"""CPU (no GPU needed): the capsule and ellipsoid rules of cvx_world_brush (cpuvox_amd/csrc/cvx_brush.h), compiled for the host through
tests/shape_rules.cpp, against tests/shapemodel.py, which evaluates the predicates of include/cpuvox_gpu.h voxel by voxel and knows no spans.

- StrokeSpan on every column of small grids: random strokes, every small capsule, the named special cases.
- StrokeSpan at the limits against the predicates in Python integers, in a plain build and in one with UBSan + ASan (a stand-alone program).
- The culled walk: BrushColumn over a whole stroke list against BrushColumnOver over the list a 64-at-a-time cull leaves for each strip of 64
  columns (the kernels' cull, simulated on the host).
- cvx_world_brush's argument checks for the new shapes; the constants of the Python and C# mirrors."""
import os
import re
import subprocess

import numpy as np
import pytest

import ruleslib
import shapemodel
from cpuvox_amd import gpu
from test_world_brush_cpu import _random_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPSULE, ELLIPSOID, SPHERE, BOX = gpu.SHAPE_CAPSULE, gpu.SHAPE_ELLIPSOID, gpu.SHAPE_SPHERE, gpu.SHAPE_BOX


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("shape_rules", tmp_path_factory.mktemp("shapes"))


def _capsule(a, b, r, op=0, argb=0):
    return {"op": op, "shape": CAPSULE, "a": [int(v) for v in a], "b": [int(v) for v in b], "radius": int(r), "argb": argb}


def _ellipsoid(a, radii, op=0, argb=0):
    return {"op": op, "shape": ELLIPSOID, "a": [int(v) for v in a], "b": [int(v) for v in radii], "argb": argb}


def _sphere(a, r, op=0, argb=0):
    return {"op": op, "shape": SPHERE, "a": [int(v) for v in a], "radius": int(r), "argb": argb}


def _words(s):
    r = gpu.strokes_array([s])[0]
    return [int(r["op"]), int(r["shape"]), *[int(v) for v in r["a"]], *[int(v) for v in r["b"]], int(np.int32(np.uint32(r["argb"]))), int(r["pad_"])]


def _spans(rules, tmp_path, strokes, n):
    """StrokeSpan of each stroke on every column of the n^3 grid: an array (strokes, n, n, 2)."""
    src, dst = tmp_path / "spans.bin", tmp_path / "spans.out"
    words = []
    for s in strokes:
        words += [n, 0, n, 0, n] + _words(s)
    src.write_bytes(np.array(words, dtype=np.int64).astype(np.int32).tobytes())
    subprocess.check_call([rules, "spans", str(src), str(dst)])
    return np.frombuffer(dst.read_bytes(), dtype=np.int32).reshape(len(strokes), n, n, 2)


def _mask_of_spans(spans, n):
    y = np.arange(n).reshape(1, n, 1)
    return (y >= spans[:, :, 0][:, None, :]) & (y < spans[:, :, 1][:, None, :])  # (x, y, z)


def _check_spans(rules, tmp_path, strokes, n):
    got = _spans(rules, tmp_path, strokes, n)
    bad = []
    for k, s in enumerate(strokes):
        want = shapemodel.stroke_mask(s, (n, n, n))
        if not (_mask_of_spans(got[k], n) == want).all():
            bad.append(k)
        empty = ~want.any(axis=1)
        assert (got[k][empty][:, 0] >= got[k][empty][:, 1]).all()
    assert not bad, f"{len(bad)} of {len(strokes)} strokes differ from the model; first: {strokes[bad[0]]}"
    return got


def test_stroke_span_matches_the_model_on_random_strokes(rules, tmp_path):
    rng = np.random.default_rng(1617)
    n, strokes = 48, []
    for k in range(3000):
        if k % 2:
            strokes.append(_capsule(rng.integers(-8, n + 8, size=3), rng.integers(-8, n + 8, size=3), rng.integers(0, 10)))
        else:
            strokes.append(_ellipsoid(rng.integers(-8, n + 8, size=3), rng.integers(1, 10, size=3)))
    _check_spans(rules, tmp_path, strokes, n)


def test_every_small_capsule(rules, tmp_path):
    n, strokes = 16, []
    for dx in range(-3, 4):
        for dy in range(-3, 4):
            for dz in range(-3, 4):
                for r in range(5):
                    strokes.append(_capsule((8, 8, 8), (8 + dx, 8 + dy, 8 + dz), r))
    assert len(strokes) == 7 ** 3 * 5
    _check_spans(rules, tmp_path, strokes, n)


def test_named_special_cases(rules, tmp_path):
    n = 40
    point = [_capsule((20, 19, 21), (20, 19, 21), r) for r in range(0, 12)]
    spheres = [_sphere((20, 19, 21), r) for r in range(0, 12)]
    same = [_ellipsoid((20, 19, 21), (r, r, r)) for r in range(1, 12)]
    lines = [_capsule((20, 5, 21), (20, 33, 21), 3), _capsule((20, 33, 21), (20, 5, 21), 0),       # vertical
             _capsule((4, 19, 21), (35, 19, 21), 4), _capsule((20, 19, 36), (20, 19, 2), 2),      # axis-parallel
             _capsule((5, 5, 5), (34, 34, 34), 3), _capsule((34, 5, 34), (5, 34, 5), 5), _capsule((5, 20, 5), (30, 20, 30), 2),  # 45 degrees
             _capsule((5, 5, 5), (34, 34, 34), 0), _capsule((3, 30, 4), (33, 10, 19), 0), _capsule((2, 2, 2), (37, 9, 16), 0),   # r = 0
             _capsule((-30, 10, 20), (70, 30, 20), 6), _capsule((20, -50, 20), (21, 90, 22), 4)]
    flat = [_ellipsoid((20, 19, 21), radii) for radii in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 15), (1, 15, 1), (15, 1, 1), (1, 1, 1), (17, 3, 8))]
    got = _check_spans(rules, tmp_path, point + spheres + same + lines + flat, n)
    assert (got[:12] == got[12:24]).all(), "a capsule with a == b is the sphere"
    assert (got[24:35] == got[13:24]).all(), "an ellipsoid with equal radii is the sphere"
    # r = 0: exactly the voxels whose centre the segment passes through
    diagonal = shapemodel.stroke_mask(lines[7], (n, n, n))
    assert diagonal.sum() == 30 and all(diagonal[k, k, k] for k in range(5, 35))
    assert shapemodel.stroke_mask(lines[8], (n, n, n)).sum() == 6   # gcd(30, 20, 15) + 1
    assert shapemodel.stroke_mask(lines[9], (n, n, n)).sum() == 8   # gcd(35, 7, 14) + 1


# ---- the limits --------------------------------------------------------------------------------------------------------------------------------

BIG = 1 << 30
DIM_Y = 1 << 32  # (so that nothing of a stroke near y = 2^30 is clipped away)


def _limit_strokes():
    out = []
    for sx in (1, -1):
        for sz in (1, -1):
            for d in ((8191, 8191, 8191), (8191, -8191, 8191), (-8191, 8191, 1), (1, 8191, 0), (8191, 0, -8191), (0, 8191, 0), (8191, 1, 3), (-5000, 37, 8191)):
                for r in (8191, 8190, 0, 1, 100):
                    a = (sx * BIG, BIG, sz * BIG)
                    out.append(_capsule(a, [a[i] + d[i] for i in range(3)], r))
    out.append(_capsule((-BIG, -BIG, -BIG), (-BIG + 8191, -BIG + 8191, -BIG + 8191), 8191))  # below the world: nothing, and nothing overflows
    for radii in ((1024, 1024, 1024), (1, 1024, 1024), (1024, 1, 1024), (1024, 1024, 1), (1, 1, 1024), (1, 1024, 1), (1024, 1, 1), (1023, 1024, 1022), (1024, 7, 333)):
        for c in ((0, 5000, 0), (2**31 - 1, 2**31 - 1, -2**31), (-2**31, 2000, 2**31 - 1)):
            out.append(_ellipsoid(c, radii))
    return out


def _footprint(s):
    a, b = s["a"], s["b"]
    if s["shape"] == CAPSULE:
        return [(min(a[i], b[i]) - s["radius"], max(a[i], b[i]) + s["radius"] + 1) for i in range(3)]
    return [(a[i] - b[i], a[i] + b[i] + 1) for i in range(3)]


def _limit_columns(rng, s, count=24):
    """Sampled columns of the footprint (a capsule's: near its axis, where the column is not empty, and anywhere), its corners, and columns just outside."""
    (x0, x1), _, (z0, z1) = _footprint(s)
    cols = [(int(rng.integers(x0, x1)), int(rng.integers(z0, z1))) for _ in range(count // 3)]
    a, b = s["a"], s["b"]
    for _ in range(count - count // 3):
        if s["shape"] == CAPSULE:
            t, r = rng.uniform(-0.05, 1.05), s["radius"]
            cx, cz = a[0] + t * (b[0] - a[0]) + rng.uniform(-1.02, 1.02) * r, a[2] + t * (b[2] - a[2]) + rng.uniform(-1.02, 1.02) * r
        else:
            ang, rad = rng.uniform(0, 2 * np.pi), rng.choice([1.0, 0.999, 1.001, rng.uniform(0, 1)])
            cx, cz = a[0] + rad * b[0] * np.cos(ang), a[2] + rad * b[2] * np.sin(ang)
        cols.append((min(max(int(round(cx)), x0), x1 - 1), min(max(int(round(cz)), z0), z1 - 1)))
    cols += [(x0, z0), (x1 - 1, z1 - 1), (x0, z1 - 1), (a[0], a[2])]
    outside = [(x0 - 1, a[2]), (x1, a[2]), (a[0], z0 - 1), (a[0], z1), (x0 - 1, z0 - 1), (x1 + 5, z1 + 7)]
    return cols, outside


def _limit_cases(rng):
    cases = []
    for s in _limit_strokes():
        cols, outside = _limit_columns(rng, s)
        cases.append((s, cols, outside))
    return cases


def _run_points(program, tmp_path, cases):
    src, dst = tmp_path / "points.bin", tmp_path / "points.out"
    words = []
    for s, cols, outside in cases:
        words += [DIM_Y] + _words(s) + [len(cols) + len(outside)]
        for cx, cz in cols + outside:
            words += [cx, cz]
    src.write_bytes(np.array(words, dtype=np.int64).tobytes())
    subprocess.check_call([program, "points", str(src), str(dst)])
    return np.frombuffer(dst.read_bytes(), dtype=np.int64).reshape(-1, 2)


def _probe_ys(s):
    """Where a column of the stroke's footprint would be covered if it were covered anywhere near the shape's middle."""
    a, b = s["a"], s["b"]
    if s["shape"] == ELLIPSOID:
        return [a[1]]
    ys = set()
    for k in range(65):
        y = a[1] + (k * (b[1] - a[1])) // 64
        ys.update((y - 1, y, y + 1))
    return sorted(ys)


def _check_points(cases, got):
    at, non_empty = 0, 0
    for s, cols, outside in cases:
        below = s["a"][1] < 0
        for k, (cx, cz) in enumerate(cols + outside):
            lo, hi = int(got[at][0]), int(got[at][1])
            at += 1
            if k >= len(cols) or below:
                assert lo >= hi, f"{s}: column {(cx, cz)} outside the footprint (or below the world) has the span {lo, hi}"
                continue
            if lo < hi:
                non_empty += 1
                inside = [shapemodel.inside(s, cx, y, cz) for y in (lo - 1, lo, hi - 1, hi)]
                assert inside == [False, True, True, False], f"{s}: column {(cx, cz)}: span {lo, hi}, the predicate around its ends {inside}"
            else:
                hits = [y for y in _probe_ys(s) if shapemodel.inside(s, cx, y, cz)]
                assert not hits, f"{s}: column {(cx, cz)} has no span, but the predicate holds at y = {hits[:3]}"
    assert at == len(got)
    return non_empty


def test_spans_at_the_limits_match_the_integer_predicates(rules, tmp_path):
    cases = _limit_cases(np.random.default_rng(8191))
    got = _run_points(rules, tmp_path, cases)
    non_empty = _check_points(cases, got)
    assert sum(len(c[1]) for c in cases) > 300 and non_empty > 2000, non_empty


def test_the_limits_under_ubsan_and_asan(tmp_path):
    """The same program built a second time with the sanitizers and run stand-alone on the limits: a signed overflow at the documented limits
    (or a read out of bounds) ends it with an error."""
    program = ruleslib.build("shape_rules", tmp_path, "-g", "-DSHAPE_RULES_NO_LIBRARY", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", link_library=False)
    cases = _limit_cases(np.random.default_rng(8191))
    got = _run_points(program, tmp_path, cases)
    assert _check_points(cases, got) > 2000


# ---- the culled walk ----------------------------------------------------------------------------------------------------------------------------

def _mixed_strokes(rng, count, x0, z0, size_x, size_z, dim_y):
    out = []
    for _ in range(count):
        op, argb = int(rng.integers(0, 3)), int(rng.integers(0, 2**32))
        c = [x0 + int(rng.integers(-3, size_x + 3)), int(rng.integers(-3, dim_y + 3)), z0 + int(rng.integers(-3, size_z + 3))]
        kind = int(rng.integers(0, 4))
        if kind == 0:
            s = {"op": op, "shape": BOX, "a": c, "b": [c[0] + int(rng.integers(0, 6)), c[1] + int(rng.integers(0, 9)), c[2] + int(rng.integers(0, 6))], "argb": argb}
        elif kind == 1:
            s = _sphere(c, rng.integers(0, 5), op, argb)
        elif kind == 2:
            s = _capsule(c, [c[i] + int(rng.integers(-9, 10)) for i in range(3)], rng.integers(0, 4), op, argb)
        else:
            s = _ellipsoid(c, rng.integers(1, 7, size=3), op, argb)
        out.append(s)
    return out


@pytest.mark.parametrize("size_x,size_z,count,seed", [(8, 64, 1, 1), (7, 37, 64, 2), (5, 100, 65, 3), (3, 128, 129, 4), (9, 24, 300, 5), (16, 16, 200, 6)])
def test_the_culled_walk_equals_the_whole_list(rules, tmp_path, size_x, size_z, count, seed):
    rng = np.random.default_rng(seed)
    dim_y, x0, z0 = 32, int(rng.integers(0, 50)), int(rng.integers(0, 50))
    stride = int(rng.choice([1, 32]))
    strokes = _mixed_strokes(rng, count, x0, z0, size_x, size_z, dim_y)
    words = [dim_y, x0, z0, size_x, size_z, stride, len(strokes)]
    for s in strokes:
        words += _words(s)
    base = 32
    for _ in range(size_x * size_z):
        runs, colours, _, _ = _random_column(rng, dim_y)
        words += ruleslib.column_words(base, runs, colours)
        base += stride * (len(colours) + 1)
    src = tmp_path / "cull.bin"
    src.write_bytes(np.array(words, dtype=np.int64).astype(np.int32).tobytes())
    columns, strips, wrapped, listed, mismatches = [int(v) for v in subprocess.check_output([rules, "cull", str(src)], text=True).split()]
    assert columns == size_x * size_z and strips == (columns + 63) // 64
    assert mismatches == 0, f"{mismatches} of {columns} columns differ between the whole list and the culled one"
    if size_z % 64:
        assert wrapped > 0
    if count >= 64:
        assert 0 < listed < strips * count, "the cull must drop strokes here, and keep some"


# ---- arguments and mirrors ----------------------------------------------------------------------------------------------------------------------

def test_brush_validates_the_new_shapes_without_a_world(rules):
    """A context without a device or world: a violated limit is CVX_ERR_INVALID_ARGUMENT (-1) naming the stroke, a valid capsule and ellipsoid
    get as far as CVX_ERR_NOT_READY (-3), the codes 2 .. 15 stay bad shapes."""
    text = subprocess.check_output([rules, "args"], text=True)
    limits, shapes, last = text.split("|")
    codes = [int(v) for v in limits.split()]
    assert codes[:2] == [-3, -3] and codes[2:] == [-1] * (2 + 3 * 7), codes
    assert [int(v) for v in shapes.split()] == [-1] * 14
    assert last.split()[0] == "-1" and "stroke 2" in last and "capsule radius" in last, last


def test_shape_constants_match_the_header():
    header = open(os.path.join(ROOT, "include", "cpuvox_gpu.h")).read()
    want = {name: int(value) for name, value in re.findall(r"CVX_SHAPE_([A-Z]+) = (\d+)", header)}
    assert want == {"BOX": 0, "SPHERE": 1, "CAPSULE": 16, "ELLIPSOID": 17}
    assert {n: getattr(gpu, "SHAPE_" + n) for n in want} == want
    cs = open(os.path.join(ROOT, "host", "csharp", "CpuVoxGpu.cs")).read()
    assert {name: int(value) for name, value in re.findall(r"CVX_SHAPE_([A-Z]+) = (\d+)", cs)} == want
    a = gpu.strokes_array([_capsule((1, 2, 3), (4, 5, 6), 7, gpu.BRUSH_CARVE), _ellipsoid((1, 2, 3), (4, 5, 6), gpu.BRUSH_PAINT, 0xFF010203)])
    assert a["shape"].tolist() == [16, 17] and a["b"].tolist() == [[4, 5, 6], [4, 5, 6]] and a["pad_"].tolist() == [7, 0]
    assert a["argb"].tolist() == [0, 0xFF010203] and a.dtype.itemsize == 40
