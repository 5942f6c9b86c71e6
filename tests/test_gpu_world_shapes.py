"""GPU: the capsule and ellipsoid shapes of cvx_world_brush, and the per-wave cull of the stroke list that both brush kernels begin with.

The strokes are applied to a context and, independently, to the dense numpy volume by tests/shapemodel.py, which evaluates each shape's
predicate voxel by voxel.  The context's world, read back whole (read_voxels: solid and colour, element for element), must equal the model; the
first test also renders it against a world rebuilt from the model (the world, poses and helpers of tests/test_gpu_world_edit.py).  The cull must
not change a byte: its tests use stroke counts around the 64-stroke ballot step, a list that fills the wave's list to the last slot, and
footprints that end at the edges of a wave's strip of 64 columns."""
import numpy as np
import pytest

import pickmodel
import shapemodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _box, _check_picks, _dense, _mixed, _sphere, _world
from test_gpu_world_edit import DIMS, _check_world, _context, _frames, _terrain
from test_gpu_world_pieces import GROUND, _report

pytestmark = pytest.mark.gpu

FILL, CARVE, PAINT = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT
CAPSULE, ELLIPSOID = gpu.SHAPE_CAPSULE, gpu.SHAPE_ELLIPSOID
OPS = (FILL, CARVE, PAINT)


def _capsule(op, a, b, r, argb=0):
    return {"op": op, "shape": CAPSULE, "a": a, "b": b, "radius": r, "argb": argb}


def _ellipsoid(op, c, radii, argb=0):
    return {"op": op, "shape": ELLIPSOID, "a": c, "b": radii, "argb": argb}


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    colour = _dense(solid)
    return solid, colour, _world(solid, colour)


def _model(solid, colour, strokes):
    s, c = solid.copy(), colour.copy()
    shapemodel.apply_strokes(s, c, gpu.strokes_array(strokes))
    return s, c


def _assert_equals_model(ctx, solid, colour, label):
    argb, is_solid = ctx.read_voxels((0, 0, 0), DIMS)
    want_solid, want_argb = solid.transpose(0, 2, 1), colour.transpose(0, 2, 1)
    bad = is_solid != want_solid
    assert not bad.any(), f"{label}: {int(bad.sum())} voxels differ in solidity, first (x, z, y) {np.argwhere(bad)[0].tolist()}"
    bad = argb != want_argb
    assert not bad.any(), f"{label}: {int(bad.sum())} voxels differ in colour, first (x, z, y) {np.argwhere(bad)[0].tolist()}"


def _levels(ctx):
    return [ctx.read_level(k)[0] for k in range(6)]


def _footprint(s):
    """The unclipped column box (x0, x1, z0, z1), exclusive ends, of one record of a STROKE_DTYPE array: the rule of include/cpuvox_gpu.h."""
    a, b, r = [int(v) for v in s["a"]], [int(v) for v in s["b"]], int(s["pad_"])
    per_axis = {0: lambda i: (a[i], b[i]), 1: lambda i: (a[i] - b[0], a[i] + b[0] + 1), CAPSULE: lambda i: (min(a[i], b[i]) - r, max(a[i], b[i]) + r + 1),
                ELLIPSOID: lambda i: (a[i] - b[i], a[i] + b[i] + 1)}[int(s["shape"])]
    return per_axis(0) + per_axis(2)


def _rectangle(strokes):
    """The brush's rectangle (x0, z0, sizeX, sizeZ) at levelCount 0: the union of the footprints, clipped to the world."""
    boxes = [_footprint(s) for s in gpu.strokes_array(strokes)]
    x0, x1 = max(min(b[0] for b in boxes), 0), min(max(b[1] for b in boxes), DIMS[0])
    z0, z1 = max(min(b[2] for b in boxes), 0), min(max(b[3] for b in boxes), DIMS[2])
    return x0, z0, x1 - x0, z1 - z0


def _size_z(strokes):
    return _rectangle(strokes)[3]


# every kind of change with the new shapes, boxes and spheres in between so that order matters
STROKES = [
    _capsule(CARVE, (20, 40, 30), (60, 0, 70), 5),                      # a diagonal tunnel through the slabs and the terrain down to y = 0
    _capsule(FILL, (90, 0, 20), (90, 55, 20), 3, 0xFF2040F0),           # vertical: a pillar deeper than its colour blocks
    _capsule(FILL, (70, 45, 100), (110, 45, 100), 2, 0xFFA0A000),       # axis-parallel: a floating beam
    _capsule(PAINT, (50, 10, 50), (80, 36, 62), 6, 0xFF808080),         # paint over mixed ground (air stays air)
    _ellipsoid(FILL, (100, 30, 60), (14, 4, 9), 0xFF00FFFF),            # flat, with a smaller one carved out of it
    _ellipsoid(CARVE, (100, 30, 60), (8, 2, 5)),
    _ellipsoid(FILL, (24, 30, 110), (3, 20, 5), 0xFF10E010),            # tall
    _box(FILL, (30, 18, 90), (44, 30, 104), 0xFF0000FF),                # order matters: a box, a sphere carved out of it, a capsule laid through the
    _sphere(CARVE, (37, 24, 97), 5),                                    #   hole, an ellipsoid painted over all of it, a box cut off the end
    _capsule(FILL, (31, 24, 91), (43, 24, 103), 1, 0xFF00FF00),
    _ellipsoid(PAINT, (37, 24, 97), (9, 4, 9), 0xFFFF00FF),
    _box(CARVE, (41, 18, 100), (44, 30, 104)),
    _capsule(FILL, (120, 20, 120), (140, 30, 135), 4, 0xFF123456),      # one end outside the world
    _capsule(CARVE, (300, 10, 10), (320, 20, 30), 5),                   # wholly outside: does nothing
    _sphere(FILL, (126, 50, 3), 6, 0xFF654321),
]
# levelCount 0 (the rectangle is not rounded): footprints whose union is 37 and 100 columns wide in z, so that the 64-column strips wrap rows
NARROW = [_capsule(CARVE, (10, 20, 41), (50, 3, 71), 3), _ellipsoid(FILL, (30, 30, 56), (12, 3, 7), 0xFF00FFFF), _sphere(CARVE, (30, 30, 56), 2),
          _capsule(FILL, (44, 0, 60), (44, 50, 60), 2, 0xFF2040F0), _box(PAINT, (12, 0, 40), (40, 20, 70), 0xFF808080)]
WIDE = [_capsule(CARVE, (5, 30, 14), (100, 2, 105), 4), _ellipsoid(FILL, (60, 40, 60), (20, 5, 30), 0xFFA0A000), _capsule(PAINT, (7, 12, 100), (90, 12, 20), 3, 0xFF808080),
        _ellipsoid(CARVE, (60, 40, 60), (10, 6, 12)), _sphere(FILL, (60, 40, 60), 3, 0xFF0000FF)]


@pytest.mark.parametrize("level_count,strokes,size_z", [(5, STROKES, None), (3, STROKES, None), (0, NARROW, 37), (0, WIDE, 100)])
def test_shapes_equal_the_model_and_its_rebuild(world_a, level_count, strokes, size_z):
    solid_a, colour_a, ws_a = world_a
    if size_z is not None:
        assert _size_z(strokes) == size_z
    solid_b, colour_b = _model(solid_a, colour_a, strokes)
    ws_b = _world(solid_b, colour_b)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        assert ctx.brush(strokes, level_count) > 0.0
        _assert_equals_model(ctx, solid_b, colour_b, f"levelCount {level_count}")
        visited = _check_world(ctx, _mixed(ws_b, ws_a, level_count), frames, f"shapes, levelCount {level_count}")
        assert (visited > 0).all(), f"the frames reach LOD visits {visited.tolist()}: every level must be drawn"
    finally:
        ctx.close()


def test_degenerate_shapes_are_the_sphere(world_a):
    _, _, ws_a = world_a
    c = (61, 17, 43)
    lists = [[_sphere(CARVE, c, 9), _sphere(FILL, (20, 30, 99), 4, 0xFF112233), _sphere(PAINT, (90, 12, 30), 0, 0xFF445566)],
             [_capsule(CARVE, c, c, 9), _capsule(FILL, (20, 30, 99), (20, 30, 99), 4, 0xFF112233), _capsule(PAINT, (90, 12, 30), (90, 12, 30), 0, 0xFF445566)],
             [_ellipsoid(CARVE, c, (9, 9, 9)), _ellipsoid(FILL, (20, 30, 99), (4, 4, 4), 0xFF112233), _sphere(PAINT, (90, 12, 30), 0, 0xFF445566)]]
    levels = []
    for strokes in lists:
        ctx = _context(ws_a)
        try:
            ctx.brush(strokes, 5)
            levels.append(_levels(ctx))
        finally:
            ctx.close()
    assert levels[1] == levels[0], "capsules with a == b leave other bytes than the spheres"
    assert levels[2] == levels[0], "ellipsoids with equal radii leave other bytes than the spheres"


def _strokes_over_a_column(rng, count, cx, cz):
    """Small boxes and spheres and a few capsules whose footprints all hold the column (cx, cz); the ops cycle and every stroke has a colour of
    its own, so a stroke lost, doubled or out of order changes a voxel."""
    out = []
    for k in range(count):
        op, argb = OPS[k % 3], 0xFF000000 | (k * 4099 + 17) & 0xFFFFFF
        ox, oz, y = int(rng.integers(-2, 3)), int(rng.integers(-2, 3)), int(rng.integers(1, 62))
        if k % 16 == 5:
            a = (cx + ox, y, cz + oz)
            out.append(_capsule(op, a, (a[0] + int(rng.integers(-4, 5)), y + int(rng.integers(-6, 7)), a[2] + int(rng.integers(-4, 5))), 3, argb))
        elif k % 2:
            out.append(_sphere(op, (cx + ox, y, cz + oz), int(rng.integers(3, 6)), argb))
        else:
            out.append(_box(op, (cx + min(ox, 0), y, cz + min(oz, 0)), (cx + max(ox, 0) + 1, y + int(rng.integers(1, 7)), cz + max(oz, 0) + 1), argb))
    return out


@pytest.mark.parametrize("count", [63, 64, 65, 128, 129, 4096])
def test_the_cull_keeps_every_stroke_in_order(world_a, count):
    """All footprints overlap one strip of 64 columns: the list grows by whole and partial ballots (63 .. 129 strokes) and, with 4096 strokes over
    one column, to its last slot."""
    solid_a, colour_a, ws_a = world_a
    strokes = _strokes_over_a_column(np.random.default_rng(count), count, 40, 20)
    solid_b, colour_b = _model(solid_a, colour_a, strokes)
    assert (solid_b != solid_a).any()
    ctx = _context(ws_a)
    try:
        ctx.brush(strokes, 0)
        _assert_equals_model(ctx, solid_b, colour_b, f"{count} strokes over one column")
    finally:
        ctx.close()


RECT = (8, 16, 6, 100)  # x 8 .. 13, z 16 .. 115 at levelCount 0: pinned by two anchor boxes, and no other footprint may reach outside it


def _strip_column(i):
    """Column i of RECT in the blob's order, which is the kernels' thread order: strip k is the columns 64 k .. 64 k + 63."""
    return RECT[0] + i // RECT[3], RECT[1] + i % RECT[3]


def _edge_strokes(strip):
    """Strokes that meet strip `strip` of RECT in its first or in its last column only, and strokes one column short of it, which miss it:
    [(stroke, the column it must cover, whether that column belongs to the strip)].  Boxes of one column; spheres and capsules that reach the
    column with the very end of their footprint, where their span is one voxel."""
    out = []
    for i, step in ((64 * strip, -1), (64 * strip + 63, 1)):
        (x, z), (xo, zo) = _strip_column(i), _strip_column(i + step)
        assert xo == x and zo == z + step, "the strip's edge and its neighbour lie in one row"
        y = 30 + 2 * len(out)
        for shift, column, inside in ((0, (x, z), True), (step, (xo, zo), False)):
            c = z + shift
            out.append((_box(FILL, (x, y, c), (x + 1, y + 2, c + 1), 0xFF0000A0 + len(out)), column, inside))
            out.append((_sphere(FILL, (x, y + 3, c + 2 * step), 2, 0xFF00A000 + len(out)), column, inside))
            out.append((_capsule(FILL, (x, y + 6, c + step), (x, y + 8, c + 3 * step), 1, 0xFFA00000 + len(out)), column, inside))
    return out


def test_the_cull_at_the_edges_of_a_strip(world_a):
    """levelCount 0 and two anchor boxes make the rectangle RECT, 100 columns wide, so strip 5 (columns 320 .. 383) is row 11, z 36 .. 99, and strip 4
    (256 .. 319) wraps: row 10, z 72 .. 115, then row 11, z 16 .. 35.  Footprints end exactly at the first and the last column of either strip,
    covering a voxel there, and one column short of them; one stroke touches only the second row of the wrapped strip.  A stroke the cull dropped at
    a strip's edge would leave its voxel unchanged there."""
    solid_a, colour_a, ws_a = world_a
    anchors = [_box(PAINT, (8, 0, 16), (9, 1, 17), 0xFF010101), _box(PAINT, (13, 0, 115), (14, 1, 116), 0xFF020202)]
    edges = _edge_strokes(5) + _edge_strokes(4)
    second_row = _box(FILL, (11, 50, 20), (12, 55, 25), 0xFF00C0C0)
    strokes = anchors + [s for s, _, _ in edges] + [second_row, _ellipsoid(FILL, (11, 44, 60), (2, 3, 40), 0xFF707070)]
    assert _rectangle(strokes) == RECT
    assert [_strip_column(i) for i in (256, 319, 320, 383)] == [(10, 72), (11, 35), (11, 36), (11, 99)]
    strips = {k: {_strip_column(i) for i in range(64 * k, 64 * k + 64)} for k in (4, 5)}
    for k, (stroke, column, inside) in enumerate(edges):
        strip = strips[5 if k < len(edges) // 2 else 4]
        x0, x1, z0, z1 = _footprint(gpu.strokes_array([stroke])[0])
        met = {(x, z) for x in range(x0, x1) for z in range(z0, z1)} & strip
        assert met == ({column} if inside else set()), f"{stroke} meets its strip in {sorted(met)}"
        assert (column in strip) == inside
        assert shapemodel.stroke_mask(gpu.strokes_array([stroke])[0], DIMS)[column[0], :, column[1]].any(), f"{stroke} covers no voxel of column {column}"
    x0, x1, z0, z1 = _footprint(gpu.strokes_array([second_row])[0])
    met = {(x, z) for x in range(x0, x1) for z in range(z0, z1)} & strips[4]
    assert met and all(x == 11 for x, _ in met), "a stroke in the wrapped strip's second row only"
    solid_b, colour_b = _model(solid_a, colour_a, strokes)
    for stroke, column, _ in edges:
        assert solid_b[column[0], :, column[1]].sum() > solid_a[column[0], :, column[1]].sum()
    ctx = _context(ws_a)
    try:
        ctx.brush(strokes, 0)
        _assert_equals_model(ctx, solid_b, colour_b, "strokes at the strips' edges")
        # a rectangle wider than a strip (levelCount 5: x 0 .. 31, z 0 .. 127) with strokes in one corner and along one edge only: most waves have
        # an empty list and re-emit their columns as they are (the rectangle holds RECT, whose levels 1 .. 5 the call above left stale)
        corner = [_capsule(CARVE, (3, 20, 2), (6, 4, 9), 2), _ellipsoid(FILL, (4, 40, 5), (3, 2, 4), 0xFF334455), _box(PAINT, (2, 0, 2), (4, 9, 118), 0xFF556677)]
        ctx.brush(corner, 5)
        solid_c, colour_c = _model(solid_b, colour_b, corner)
        _assert_equals_model(ctx, solid_c, colour_c, "strokes in one corner of the rectangle")
        _check_world(ctx, _world(solid_c, colour_c), _frames(ws_a)[1:2], "strokes in one corner", fresh=False)
    finally:
        ctx.close()


def test_thousands_of_scattered_strokes(world_a):
    """4096 spheres of radius 2 in one call (CVX_BRUSH_MAX_STROKES of them) and then 1024 short capsules in one call, scattered over the whole
    world, equal the model; a second context that takes the same 5120 strokes in 64 calls of 80 reads back equal.  (5120 strokes do not fit in
    one call.)  A third context takes 3072 of the spheres and the 1024 capsules interleaved in ONE call of 4096 strokes, so that scattered spheres
    and capsules share a cull and a list."""
    solid_a, colour_a, ws_a = world_a
    rng = np.random.default_rng(4096)
    spheres = [_sphere(OPS[k % 3], [int(v) for v in rng.integers((0, 0, 0), DIMS)], 2, 0xFF000000 | (k * 2731 + 5) & 0xFFFFFF) for k in range(4096)]
    capsules = []
    for k in range(1024):
        a = [int(v) for v in rng.integers((-2, 0, -2), (DIMS[0] + 2, DIMS[1], DIMS[2] + 2))]
        capsules.append(_capsule(OPS[(k + 1) % 3], a, [a[i] + int(rng.integers(-6, 7)) for i in range(3)], int(rng.integers(0, 3)), 0xFF000000 | (k * 6151 + 9) & 0xFFFFFF))
    solid_b, colour_b = _model(solid_a, colour_a, spheres + capsules)
    one, many = _context(ws_a), _context(ws_a)
    try:
        assert one.brush(spheres, 5) > 0.0 and one.brush(capsules, 5) > 0.0
        _assert_equals_model(one, solid_b, colour_b, "4096 spheres, then 1024 capsules")
        both = spheres + capsules
        for k in range(0, len(both), 80):
            many.brush(both[k:k + 80], 5)
        _assert_equals_model(many, solid_b, colour_b, "the same strokes in 64 calls")
        assert _levels(many) == _levels(one)
    finally:
        one.close()
        many.close()
    mixed = []
    for k in range(1024):
        mixed += spheres[3 * k:3 * k + 3] + [capsules[k]]
    assert len(mixed) == gpu.BRUSH_MAX_STROKES
    solid_c, colour_c = _model(solid_a, colour_a, mixed)
    ctx = _context(ws_a)
    try:
        assert ctx.brush(mixed, 5) > 0.0
        _assert_equals_model(ctx, solid_c, colour_c, "3072 spheres and 1024 capsules interleaved in one call")
    finally:
        ctx.close()


def test_rejected_shapes_leave_the_world_alone(world_a):
    _, _, ws_a = world_a
    good = [_capsule(CARVE, (30, 30, 30), (60, 5, 70), 4), _ellipsoid(FILL, (90, 30, 90), (9, 4, 6), 0xFF102030)]
    far = 1 << 30
    bad = [(_capsule(CARVE, (30, 30, 30), (60, 5, 70), -1), "capsule radius"), (_capsule(CARVE, (30, 30, 30), (60, 5, 70), 8192), "capsule radius"),
           (_capsule(CARVE, (30, 30, 30), (30 + 8192, 5, 70), 4), "capsule ends"), (_capsule(CARVE, (30, 30, 30), (60, 30 - 8192, 70), 4), "capsule ends"),
           (_capsule(CARVE, (30, 30, 8192), (60, 5, 0), 4), "capsule ends"), (_capsule(CARVE, (far + 1, 30, 30), (far + 1, 5, 70), 4), "capsule end"),
           (_capsule(CARVE, (30, 30, -far - 1), (30, 5, -far - 1), 4), "capsule end"),
           (_ellipsoid(FILL, (90, 30, 90), (0, 4, 6)), "ellipsoid radius"), (_ellipsoid(FILL, (90, 30, 90), (9, 1025, 6)), "ellipsoid radius"),
           (_ellipsoid(FILL, (90, 30, 90), (9, 4, -6)), "ellipsoid radius"), (dict(good[0], shape=2), "bad shape"), (dict(good[1], shape=15), "bad shape"),
           (dict(good[1], shape=18), "bad shape")]
    ctx = _context(ws_a)
    try:
        before = _levels(ctx)
        for stroke, match in bad:
            with pytest.raises(gpu.CvxError, match=f"stroke 0: .*{match}"):
                ctx.brush([stroke], 5)
            with pytest.raises(gpu.CvxError, match=f"stroke 2: .*{match}"):
                ctx.brush(good + [stroke], 5)
        assert ctx.brush([_capsule(FILL, (-40, 10, 10), (-20, 30, 30), 5, 0xFFFFFFFF), _ellipsoid(CARVE, (64, 80, 64), (30, 10, 30))], 5) == 0.0  # outside
        assert _levels(ctx) == before
        assert ctx.edit_stats()[1:] == (0, 0)
        ctx.brush(good, 5)  # ... and the valid strokes alone are fine
        assert _levels(ctx) != before
    finally:
        ctx.close()


def test_pieces_and_picks_after_a_tunnel(world_a):
    """A tower, a capsule carved through it (its top now floats) and through the terrain: cvx_world_pieces and cvx_world_pick agree with their
    models on the model's volume."""
    solid_a, colour_a, ws_a = world_a
    strokes = [_box(FILL, (60, 0, 60), (66, 60, 66), 0xFF2040F0), _capsule(CARVE, (40, 44, 50), (90, 40, 76), 5), _capsule(CARVE, (10, 4, 10), (110, 14, 100), 3)]
    solid_b, colour_b = _model(solid_a, colour_a, strokes)
    ctx = _context(ws_a)
    try:
        for s in strokes:
            ctx.brush([s], 5)
        _assert_equals_model(ctx, solid_b, colour_b, "the tunnels")
        pieces, summary = _report(ctx, solid_b, (0, 0, 0), DIMS, GROUND, label="after the tunnel")
        assert len(pieces) >= 1, "the tower's top floats"
        _check_picks(ctx, solid_b, colour_b, np.random.default_rng(16), 2048, "after the tunnel")
        # from inside the lower tunnel along its axis, and along the upper one towards the cut tower: rays a little off either axis
        rng = np.random.default_rng(17)
        o = np.concatenate([np.float64([20.5, 5.5, 19.5]) + rng.uniform(-1.5, 1.5, size=(64, 3)), np.float64([41.0, 44.0, 50.5]) + rng.uniform(-2.0, 2.0, size=(64, 3))])
        d = np.concatenate([np.float64([100.0, 10.0, 90.0]) + rng.uniform(-4.0, 4.0, size=(64, 3)), np.float64([50.0, -4.0, 26.0]) + rng.uniform(-3.0, 3.0, size=(64, 3))])
        o, d = o.astype(np.float32), d.astype(np.float32)
        hits = np.zeros(len(o), dtype=gpu.PICK_HIT_DTYPE)
        hits["voxel"], hits["face"], hits["argb"], hits["t"] = ctx.pick(o, d, 2.0)
        model = pickmodel.pick_many(solid_b, colour_b, o, d, 2.0)
        assert pickmodel.compare_picks(hits, model, "through the tunnels") >= 0.9
        assert (model[3][model[1] >= 0] > 0.05).mean() > 0.5, "most of these rays fly some way down a tunnel before they hit"
    finally:
        ctx.close()
