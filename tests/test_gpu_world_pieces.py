"""GPU: finding and removing the floating pieces of the device-resident world (cvx_world_pieces).

Every result is compared with the dense model of tests/piecesmodel.py (scipy.ndimage.label on the numpy volume the world was built from and the
brush strokes were applied to): the four totals and the ordered list as exact integers and bytes, each call made twice with identical bytes.
REMOVE is checked by reading every level back against the host-built LOD chain of the model's result, by rendering through both kernels against
the CPU oracle, and by a second REPORT that finds nothing floating."""
import numpy as np
import pytest

import piecesmodel
import scenes
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _box, _brushed, _dense, _world
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _context, _frames
from test_world_brush_cpu import _pick_world
from test_world_pieces_cpu import GROUND, LARGEST, OUTSIDE, world_boxes

pytestmark = pytest.mark.gpu

FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE
REPORT, REMOVE = gpu.PIECES_REPORT, gpu.PIECES_REMOVE
WHOLE = ((0, 0, 0), DIMS)


def _report(ctx, solid, box_min, box_max, anchors, capacity=8192, label=""):
    """REPORT twice (identical bytes) against the model: the totals, and the first `capacity` floating pieces byte for byte."""
    want, want_summary, _ = piecesmodel.analyse(solid, box_min, box_max, anchors)
    pieces, summary, ms = ctx.world_pieces(box_min, box_max, anchors, REPORT, capacity=capacity)
    again, summary_again, _ = ctx.world_pieces(box_min, box_max, anchors, REPORT, capacity=capacity)
    assert summary == want_summary, f"{label}: {summary} != {want_summary}"
    assert len(pieces) == min(capacity, len(want)), label
    assert pieces.tobytes() == want[:capacity].tobytes(), f"{label}: first difference at piece {int(np.argmax(pieces != want[:capacity]))}"
    assert again.tobytes() == pieces.tobytes() and summary_again == summary, f"{label}: two calls differ"
    assert ms > 0.0
    return pieces, summary


def _floor():
    """The world the constructed cases are brushed into: one layer of voxels at y = 0."""
    solid = np.zeros(DIMS, dtype=bool)
    solid[:, 0, :] = True
    return solid


@pytest.fixture()
def built():
    """build(strokes) -> (ctx, solid, colour): the floor plus the strokes, on the device through cvx_world_brush and in numpy."""
    made = []

    def build(strokes):
        solid = _floor()
        colour = _dense(solid)
        ws = _world(solid, colour)
        ctx = _context(ws)
        made.append((ctx, ws))
        for at in range(0, len(strokes), gpu.BRUSH_MAX_STROKES):
            ctx.brush(strokes[at:at + gpu.BRUSH_MAX_STROKES], 5)
        solid, colour = _brushed(solid, colour, strokes)
        return ctx, solid, colour

    yield build
    for ctx, ws in made:
        ctx.close()
        ws.close()


# ---- random worlds -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((32, 128, 32), True, 3)])
def test_report_equals_the_model_on_random_worlds(dims, sparse, seed):
    """The worlds of the CPU test (records with 1 .. 3 runs, run-list columns, both colour layouts) through the real kernels: the named boxes and
    40 random boxes and anchor masks each (seed = the world's + 100)."""
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for name, (box_min, box_max, anchors) in world_boxes(dims).items():
            _report(ctx, solid, box_min, box_max, anchors, label=name)
        rng = np.random.default_rng(seed + 100)
        for k in range(40):
            box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
            box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
            if piecesmodel.clip_box(dims, box_min, box_max) is None:
                box_min = [0, 0, 0]
            _report(ctx, solid, box_min, box_max, int(rng.integers(0, 8)), capacity=int(rng.choice([0, 3, 8192])), label=f"random box {k}")
    finally:
        ctx.close()
        ws.close()


# ---- constructed cases ---------------------------------------------------------------------------------------------------------------------------

def _serpentine(size=64, y0=2):
    """One-voxel-thick strokes of a single path that winds through a size^3 volume: rows along x at every second z, joined at alternating ends,
    on every second y, the layers joined at alternating corners."""
    strokes = []
    rows = size // 2
    layers = (size - y0) // 2
    for layer in range(layers):
        y = y0 + 2 * layer
        for k in range(rows):
            strokes.append(_box(FILL, (0, y, 2 * k), (size, y + 1, 2 * k + 1), 0xFF00A0FF))
            if k + 1 < rows:
                x = size - 1 if k % 2 == 0 else 0
                strokes.append(_box(FILL, (x, y, 2 * k + 1), (x + 1, y + 1, 2 * k + 2), 0xFF00A0FF))
        if layer + 1 < layers:  # row `rows - 1` ends at x = 0 (rows is even); the next layer is walked backwards from there
            z = 2 * (rows - 1) if layer % 2 == 0 else 0
            strokes.append(_box(FILL, (0, y + 1, z), (1, y + 2, z + 1), 0xFF00A0FF))
    return strokes


def test_a_serpentine_through_the_volume_is_one_piece(built):
    """The convergence test: the path is ~65 000 voxels long and every horizontal voxel of it is a node of its own."""
    strokes = _serpentine()
    assert len(strokes) <= gpu.BRUSH_MAX_STROKES
    ctx, solid, _ = built(strokes)
    pieces, summary = _report(ctx, solid, *WHOLE, GROUND, label="serpentine")
    assert summary["floatingPieces"] == 1 and summary["anchoredPieces"] == 1 and summary["anchoredVoxels"] == DIMS[0] * DIMS[2]
    assert int(pieces[0]["voxels"]) == int(solid[:, 1:, :].sum()) > 60000
    assert pieces[0]["min"].tolist() == [0, 2, 0] and pieces[0]["max"].tolist() == [64, 63, 63] and pieces[0]["seed"].tolist() == [0, 62, 0]
    # cut the path in the middle: two pieces
    cut = _box(CARVE, (30, 32, 30), (31, 33, 31))
    ctx.brush([cut], 5)
    solid2, _ = _brushed(solid, _dense(solid), [cut])
    _, summary = _report(ctx, solid2, *WHOLE, GROUND, label="cut serpentine")
    assert summary["floatingPieces"] == 2


def test_a_checkerboard_of_single_voxels(built):
    """Most pieces per voxel: every voxel of a 20^3 checkerboard is a piece; a capacity below the count is not an error."""
    n = 20
    strokes = [_box(FILL, (40 + x, 5 + y, 40 + z), (41 + x, 6 + y, 41 + z), 0xFF102030 + x) for x in range(n) for y in range(n) for z in range(n) if (x + y + z) % 2 == 0]
    ctx, solid, _ = built(strokes)
    pieces, summary = _report(ctx, solid, *WHOLE, GROUND, label="checkerboard")
    assert summary["floatingPieces"] == n ** 3 // 2 == len(pieces) and summary["floatingVoxels"] == n ** 3 // 2
    assert (pieces["voxels"] == 1).all() and (pieces["max"] - pieces["min"] == 1).all() and (pieces["seed"] == pieces["min"]).all()
    assert pieces["seed"][:3].tolist() == [[40, 23, 40], [40, 21, 40], [40, 19, 40]]  # ascending x, z; descending y
    for capacity in (0, 1, 100, 300):  # (300: more than comes with the totals in one copy)
        few, few_summary = _report(ctx, solid, *WHOLE, GROUND, capacity=capacity, label=f"capacity {capacity}")
        assert len(few) == capacity and few_summary == summary and few.tobytes() == pieces[:capacity].tobytes()
    _report(ctx, solid, (40, 5, 40), (60, 25, 60), LARGEST, label="checkerboard, largest: the first one")


def test_edge_and_corner_contact_do_not_connect(built):
    strokes = [_box(FILL, (10, 10, 10), (14, 14, 14), 0xFF0000FF), _box(FILL, (14, 14, 10), (18, 18, 14), 0xFF00FF00),     # share the edge x = 14, y = 14
               _box(FILL, (40, 10, 40), (44, 14, 44), 0xFFFF0000), _box(FILL, (44, 14, 44), (48, 18, 48), 0xFFFFFF00),     # share one corner
               _box(FILL, (70, 10, 70), (74, 14, 74), 0xFF00FFFF), _box(FILL, (74, 13, 70), (78, 17, 74), 0xFFFF00FF)]     # share a face: one piece
    ctx, solid, _ = built(strokes)
    pieces, summary = _report(ctx, solid, *WHOLE, GROUND, label="contacts")
    assert summary["floatingPieces"] == 5 and sorted(pieces["voxels"].tolist()) == [64, 64, 64, 64, 128]
    _report(ctx, solid, (8, 8, 8), (20, 20, 20), 0, label="the two edge blocks alone")


def test_ground_outside_and_largest_anchors(built):
    strokes = [_box(FILL, (20, 1, 20), (24, 9, 24), 0xFF0000FF),       # a tower resting on the floor
               _box(FILL, (60, 20, 60), (70, 24, 70), 0xFF00FF00),     # a slab in the air ...
               _box(FILL, (69, 24, 64), (70, 40, 65), 0xFF00FF00),     # ... hanging on a pole that leaves the box below through its top
               _box(FILL, (100, 30, 100), (104, 34, 104), 0xFFFF0000), _box(FILL, (110, 30, 100), (114, 34, 104), 0xFFFF00FF)]  # two equal blocks
    ctx, solid, _ = built(strokes)
    _, summary = _report(ctx, solid, *WHOLE, GROUND, label="ground")
    assert summary["anchoredPieces"] == 1 and summary["floatingPieces"] == 3   # floor + tower; slab with its pole; the two blocks
    _, summary = _report(ctx, solid, *WHOLE, 0, label="nothing anchored")
    assert summary["anchoredPieces"] == 0 and summary["floatingPieces"] == 4
    # a box around the slab that cuts the pole: the slab is attached only through the voxel above the box
    slab_box = ((55, 15, 55), (75, 30, 75))
    pieces, summary = _report(ctx, solid, *slab_box, 0, label="slab, no anchors")
    assert summary["floatingPieces"] == 1 and int(pieces[0]["voxels"]) == 400 + 6
    _, summary = _report(ctx, solid, *slab_box, OUTSIDE, label="slab, outside")
    assert summary == {"floatingPieces": 0, "floatingVoxels": 0, "anchoredPieces": 1, "anchoredVoxels": 406}
    # ... and through a voxel beside the box
    _, summary = _report(ctx, solid, (60, 18, 60), (69, 26, 70), OUTSIDE, label="slab, cut in x")
    assert summary["floatingPieces"] == 0 and summary["anchoredPieces"] == 1
    # the tower inside a box that leaves the floor out: floating without OUTSIDE, anchored with it
    _, summary = _report(ctx, solid, (18, 1, 18), (26, 12, 26), GROUND, label="tower without its floor")
    assert summary["floatingPieces"] == 1
    _, summary = _report(ctx, solid, (18, 1, 18), (26, 12, 26), OUTSIDE, label="tower on the floor outside")
    assert summary["floatingPieces"] == 0
    # LARGEST with an exact tie: the earlier of the two equal blocks is anchored
    pieces, summary = _report(ctx, solid, (95, 25, 95), (120, 40, 110), LARGEST, label="tie")
    assert summary["anchoredPieces"] == 1 and summary["floatingPieces"] == 1 and pieces[0]["min"].tolist() == [110, 30, 100]


def test_a_split_solid_run_is_one_piece(built):
    """A foreign column whose encoding cuts one solid span into two adjacent runs (uploaded through cvx_world_set_columns)."""
    ctx, solid, _ = built([_box(FILL, (50, 10, 50), (51, 11, 51), 0xFF112233)])
    dy = DIMS[1]
    # from the top: air, 10 solid (y 20 .. 29), 10 solid (y 10 .. 19), air; colour index = the solid voxels above
    runs = [0xFFFF | ((dy - 30) << 16), 0 | (10 << 16), 10 | (10 << 16), 0xFFFF | (10 << 16)]
    blob = np.array([0, len(runs) | (10 << 16), 30, 0, *runs, 0, *[0xFF000000 | k for k in range(20)]], dtype=np.uint32).tobytes()
    ctx.set_columns(0, 80, 80, 1, 1, blob, 1)
    solid = solid.copy()
    solid[80, :, 80] = False  # (the column's floor voxel goes with the old column)
    solid[80, 10:30, 80] = True
    pieces, summary = _report(ctx, solid, *WHOLE, GROUND, label="split run")
    assert summary["floatingPieces"] == 2 and pieces[1]["seed"].tolist() == [80, 29, 80] and int(pieces[1]["voxels"]) == 20
    # a box that ends between the two halves sees the lower one hanging on the upper one
    _, summary = _report(ctx, solid, (70, 5, 70), (90, 20, 90), OUTSIDE, label="split run, cut")
    assert summary == {"floatingPieces": 0, "floatingVoxels": 0, "anchoredPieces": 1, "anchoredVoxels": 10}


def test_boxes_inside_a_structure_outside_the_world_and_a_repeating_world():
    solid = np.zeros(DIMS, dtype=bool)
    solid[:, 0, :] = True
    solid[20:100, 0:40, 20:100] = True          # a big block ...
    solid[40:60, 10:20, 40:60] = False          # ... with a cave ...
    solid[45:50, 12:16, 45:50] = True           # ... and a loose stone in it
    solid[120:128, 50:54, 120:128] = True       # a block in the corner of the world
    colour = _dense(solid)
    ws = _world(solid, colour)
    ctx = _context(ws)
    try:
        _, summary = _report(ctx, solid, (30, 5, 30), (70, 30, 70), OUTSIDE, label="inside the block")
        assert summary["floatingPieces"] == 1 and summary["floatingVoxels"] == 100 and summary["anchoredPieces"] == 1
        _, summary = _report(ctx, solid, (30, 5, 30), (70, 30, 70), 0, label="inside the block, no anchors")
        assert summary["floatingPieces"] == 2
        partly = ((110, 40, 110), (140, 70, 140))
        pieces, summary = _report(ctx, solid, *partly, GROUND, label="partly outside the world")
        assert summary["floatingPieces"] == 1 and pieces[0]["max"].tolist() == [128, 54, 128]
        with pytest.raises(gpu.CvxError, match="outside the world"):
            ctx.world_pieces((128, 0, 0), (140, 10, 10), 0)
        ctx.set_world_repeat(True)  # coordinates address the stored tile: nothing wraps
        again, _ = _report(ctx, solid, *partly, GROUND, label="repeating, partly outside")
        assert again.tobytes() == pieces.tobytes()
        _report(ctx, solid, (-10, 0, -10), (10, 64, 10), GROUND | OUTSIDE, label="repeating, across the origin")
        with pytest.raises(gpu.CvxError, match="outside the world"):
            ctx.world_pieces((128, 0, 0), (140, 10, 10), 0)
    finally:
        ctx.close()
        ws.close()


# ---- the mill ------------------------------------------------------------------------------------------------------------------------------------

def test_carving_through_the_mill_and_removing_what_floats():
    fixture = scenes.load_world("mill256")
    dims = tuple(fixture.dims)
    solid, colour = piecesmodel.decode_blob(fixture.storage(0).tobytes(), dims)
    x, y, z = np.nonzero(solid)
    ws_a = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)
    assert all(ws_a.storage(k).tobytes() == fixture.storage(k).tobytes() for k in range(6)), "the decoded fixture builds the fixture"
    slab = {"op": CARVE, "shape": gpu.SHAPE_BOX, "a": (0, 100, 0), "b": (256, 104, 256), "argb": 0}
    solid_b, colour_b = _brushed(solid, colour, [slab])
    whole = ((0, 0, 0), dims)
    want, want_summary, _ = piecesmodel.analyse(solid_b, *whole, LARGEST)
    assert len(want) > 10 and want_summary["anchoredPieces"] == 1
    solid_c, colour_c = piecesmodel.remove(solid_b, colour_b, *whole, LARGEST)
    x, y, z = np.nonzero(solid_c)
    ws_c = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour_c[x, y, z], threads=4)
    ctx = _context(ws_a)
    try:
        ctx.brush([slab], 5)
        _report(ctx, solid_b, *whole, LARGEST, label="carved mill")
        stats_before = ctx.edit_stats()
        pieces, summary, ms = ctx.world_pieces(*whole, LARGEST, REMOVE, level_count=5, capacity=4)
        assert summary == want_summary and pieces.tobytes() == want[:4].tobytes() and ms > 0.0
        _assert_levels(ctx, ws_c, ws_c, 5, "mill without its floating pieces")
        used, abandoned, spare = ctx.edit_stats()
        assert used > 0 and abandoned >= stats_before[1] and spare >= 0 and used >= abandoned
        pieces, summary = _report(ctx, solid_c, *whole, LARGEST, label="after the removal")
        assert len(pieces) == 0 and summary == {"floatingPieces": 0, "floatingVoxels": 0, "anchoredPieces": 1, "anchoredVoxels": want_summary["anchoredVoxels"]}
        # nothing floats: a second REMOVE changes nothing
        ctx.world_pieces(*whole, LARGEST, REMOVE)
        _assert_levels(ctx, ws_c, ws_c, 5, "after a REMOVE with nothing to remove")
        _check_world(ctx, ws_c, _frames(ws_c)[:2], "mill without its floating pieces")
    finally:
        ctx.close()
        for ws in (ws_a, ws_c):
            ws.close()


def test_remove_in_a_box_with_a_partial_refresh(built):
    """REMOVE with levelCount 2 in a box: only the floating pieces inside the box go, LOD 0 .. 2 are refreshed, the levels above stay."""
    strokes = [_box(FILL, (30, 10, 30), (36, 14, 36), 0xFF0000FF), _box(FILL, (33, 20, 50), (39, 22, 53), 0xFF00FF00),
               _box(FILL, (90, 10, 90), (96, 14, 96), 0xFFFF0000), _box(FILL, (5, 1, 5), (8, 30, 8), 0xFF888888)]
    ctx, solid, colour = built(strokes)
    ws_before = _world(solid, colour)
    box = ((0, 0, 0), (64, 64, 64))
    want, want_summary, _ = piecesmodel.analyse(solid, *box, GROUND)
    solid_b, colour_b = piecesmodel.remove(solid, colour, *box, GROUND)
    assert want_summary["floatingPieces"] == 2 and solid_b[92, 12, 92] and not solid_b[32, 12, 32]
    ws_after = _world(solid_b, colour_b)
    try:
        pieces, summary, _ = ctx.world_pieces(*box, GROUND, REMOVE, level_count=2)
        assert summary == want_summary and pieces.tobytes() == want.tobytes()
        _assert_levels(ctx, ws_after, ws_before, 2, "REMOVE with levelCount 2")
    finally:
        ws_before.close()
        ws_after.close()


def test_rejected_calls_leave_the_world_alone(built):
    """(No REMOVE over the format limits can be built: taking voxels out of a column lowers its colour indices and run count, and in a world the
    format can hold -- at most 32768 voxels high -- no air run next to a solid voxel passes 32767.)"""
    ctx, solid, colour = built([_box(FILL, (30, 10, 30), (36, 14, 36), 0xFF0000FF)])
    ws = _world(solid, colour)
    try:
        bad = [
            (dict(box_min=(0, 0, 0), box_max=(0, 8, 8), anchors=0), "empty"), (dict(box_min=(9, 0, 0), box_max=(8, 8, 8), anchors=0), "empty"),
            (dict(box_min=(0, 64, 0), box_max=(8, 70, 8), anchors=0), "outside the world"), (dict(box_min=(-9, 0, 0), box_max=(0, 8, 8), anchors=0), "outside the world"),
            (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), anchors=8), "anchors"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), anchors=-1), "anchors"),
            (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), anchors=0, op=2), "op"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), anchors=0, level_count=6), "levelCount"),
            (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), anchors=0, level_count=-1), "levelCount"),
            (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), anchors=0, capacity=-1), "pieceCapacity"),
        ]
        for kwargs, match in bad:
            with pytest.raises(gpu.CvxError, match=match):
                ctx.world_pieces(**{"op": REMOVE, **kwargs})
        _assert_levels(ctx, ws, ws, 5, "after the rejected calls")
        pieces, summary, _ = ctx.world_pieces(*WHOLE, GROUND, REPORT)
        assert summary["floatingPieces"] == 1
        _assert_levels(ctx, ws, ws, 5, "after a REPORT")
    finally:
        ws.close()
