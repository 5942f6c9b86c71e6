"""GPU: copying, moving and rotating voxel boxes inside the device-resident world (cvx_world_copy).

The placements are applied to world A's context and, independently, to A's dense numpy volume (tests/copymodel.py), from which B is built on the
host (host.WorldSet.from_voxels).  Read back, LOD 0 .. levelCount of the context must equal B's levels byte for byte and the levels above must be
A's; the context must render bit-identically to a fresh upload of that world and to the CPU oracle, through both kernels (the world and poses of
tests/test_gpu_world_edit.py), and picks through the copied boxes must return the model's hits."""
import numpy as np
import pytest

import copymodel
import pickmodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import STROKES, _brushed, _check_picks, _dense, _mixed, _tower_strokes, _world
from test_gpu_world_edit import DIMS, _check_world, _colour, _context, _frames, _terrain
from test_world_copy_cpu import FILL, CARVE, PAINT, REPLACE, _placement, snapshot_matters, world_cases

pytestmark = pytest.mark.gpu

CASES = world_cases(DIMS)


def _copied(solid, colour, placements):
    return copymodel.apply_copies(solid, colour, gpu.copy_placements_array(placements))


def _assert_levels(ctx, ws_new, ws_old, level_count, label):
    """LOD 0 .. level_count read back equal ws_new's levels, the levels above ws_old's, byte for byte."""
    for k in range(6):
        blob, count = ctx.read_level(k)
        ws = ws_new if k <= level_count else ws_old
        want = ws.storage(k).tobytes()
        assert count == ws.info(k).columnCount and blob == want, f"{label}: LOD {k} ({len(blob)} bytes, want {len(want)}) differs"


def _scatter(rng, count):
    """Small prefabs scattered over the world: every transform and op, some of them moving, some partly outside."""
    out = []
    for k in range(count):
        a = [int(rng.integers(0, DIMS[0] - 8)), int(rng.integers(0, 30)), int(rng.integers(0, DIMS[2] - 8))]
        size = [int(rng.integers(2, 9)), int(rng.integers(4, 30)), int(rng.integers(2, 9))]
        b = [a[i] + size[i] for i in range(3)]
        dst = [int(rng.integers(-4, DIMS[0] - 2)), int(rng.integers(-4, DIMS[1] - 6)), int(rng.integers(-4, DIMS[2] - 2))]
        out.append(_placement(a, b, dst, k % 16, (k // 16) % 4, int(k % 5 == 0)))
    return out


# the combined list of the rendering test: a prefab turned and stacked, an overlapping move, every op
COMBINED = [
    _placement((10, 0, 10), (42, 40, 26), (60, 10, 70), 1, FILL),            # a 32 x 40 x 16 piece of terrain turned onto the slabs
    _placement((10, 0, 10), (42, 40, 26), (90, 0, 20), 14, REPLACE),         # ... turned three times, mirrored and upside down
    _placement((0, 0, 64), (48, 64, 112), (8, 6, 70), 0, REPLACE, 1),        # a move that overlaps itself
    _placement((80, 0, 80), (100, 20, 100), (20, 30, 20), 5, PAINT),        # paint with another piece's colours
    _placement((64, 10, 0), (80, 50, 16), (40, 5, 40), 8, CARVE),           # carve the shape of a flipped piece
    _placement((100, 0, 100), (128, 40, 128), (115, 30, 115), 3, FILL),     # partly outside the world
]


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    colour = _dense(solid)
    return solid, colour, _world(solid, colour)


@pytest.mark.parametrize("name", sorted(CASES))
def test_each_case_reads_back_as_the_model(world_a, name):
    """Every case of the CPU test on the GPU world (all transforms and ops, overlapping moves, clipping), read back byte for byte."""
    solid_a, colour_a, ws_a = world_a
    placements = CASES[name]
    ctx = _context(ws_a)
    try:
        ms = ctx.copy(placements, 5)
        if name == "wholly outside":
            assert ms == 0.0
            _assert_levels(ctx, ws_a, ws_a, 5, name)
            return
        assert ms > 0.0
        solid_b, colour_b = _copied(solid_a, colour_a, placements)
        assert not (solid_b == solid_a).all() or not (colour_b == colour_a).all(), f"{name} changes nothing"
        ws_b = _world(solid_b, colour_b)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, name)
        finally:
            ws_b.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("transform", [0, 3, 6, 9, 12, 15])
def test_transforms_render_as_the_rebuild(world_a, transform):
    solid_a, colour_a, ws_a = world_a
    placements = CASES[f"transform {transform}"]
    ws_b = _world(*_copied(solid_a, colour_a, placements))
    ctx = _context(ws_a)
    try:
        ctx.copy(placements, 5)
        _check_world(ctx, ws_b, _frames(ws_a)[1:3], f"transform {transform}")
    finally:
        ctx.close()
        ws_b.close()


@pytest.mark.parametrize("level_count", [5, 0])
def test_copy_equals_rebuild(world_a, level_count):
    solid_a, colour_a, ws_a = world_a
    assert snapshot_matters(solid_a, colour_a, COMBINED), "the overlapping move must tell the snapshot from the half-written result"
    solid_b, colour_b = _copied(solid_a, colour_a, COMBINED)
    ws_b = _world(solid_b, colour_b)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        _check_world(ctx, ws_a, frames[:1], "A", fresh=False)
        assert ctx.copy(COMBINED, level_count) > 0.0
        _assert_levels(ctx, ws_b, ws_a, level_count, f"levelCount {level_count}")
        visited = _check_world(ctx, _mixed(ws_b, ws_a, level_count), frames, f"copied, levelCount {level_count}")
        assert (visited > 0).all(), f"the frames reach LOD visits {visited.tolist()}: every level must be drawn"
        if level_count == 5:
            _check_picks(ctx, solid_b, colour_b, np.random.default_rng(7), 4096, "copied")
            # straight down through the turned prefab and the moved block
            xs, zs = np.meshgrid(np.arange(60, 100), np.arange(20, 110, 3), indexing="ij")
            o = np.stack([xs.ravel() + 0.5, np.full(xs.size, 63.9), zs.ravel() + 0.5], axis=1).astype(np.float32)
            d = np.tile(np.float32([0.0, -1.0, 0.0]), (len(o), 1))
            vox, face, argb, t = ctx.pick(o, d, 100.0)
            got = np.zeros(len(o), dtype=gpu.PICK_HIT_DTYPE)
            got["voxel"], got["face"], got["argb"], got["t"] = vox, face, argb, t
            assert pickmodel.compare_picks(got, pickmodel.pick_many(solid_b, colour_b, o, d, 100.0), "down the copies") == 1.0
    finally:
        ctx.close()
        ws_b.close()


def test_scatter_of_64_placements(world_a):
    solid_a, colour_a, ws_a = world_a
    placements = _scatter(np.random.default_rng(64), 64)
    solid_b, colour_b = _copied(solid_a, colour_a, placements)
    ws_b = _world(solid_b, colour_b)
    ctx = _context(ws_a)
    try:
        assert ctx.copy(placements, 5) > 0.0
        _assert_levels(ctx, ws_b, ws_a, 5, "scatter")
        _check_world(ctx, ws_b, _frames(ws_a)[1:3], "scatter")
    finally:
        ctx.close()
        ws_b.close()


def test_copy_after_a_brush_and_a_compaction(world_a):
    """Sources in edit tails and run lists: brushes move blocks to the tails and make listed columns, a copy reads them; after a compaction a
    second copy reads the new layout."""
    solid_a, colour_a, ws_a = world_a
    strokes = STROKES + _tower_strokes(np.random.default_rng(9), 16)
    first = [_placement((84, 40, 70), (101, 60, 90), (10, 30, 10), 5, REPLACE, 1),     # the four-run slab, moved and mirrored
             _placement((20, 0, 20), (80, 64, 80), (40, 0, 60), 2, FILL)]              # towers with their own colours, turned
    second = [_placement((0, 0, 0), (64, 64, 64), (32, 2, 32), 11, REPLACE, 1),
              _placement((10, 30, 10), (27, 50, 30), (100, 40, 100), 4, PAINT)]
    solid, colour = _brushed(solid_a, colour_a, strokes)
    solid, colour = _copied(solid, colour, first)
    ws_mid = _world(solid, colour)
    solid, colour = _copied(solid, colour, second)
    ws_b = _world(solid, colour)
    ctx = _context(ws_a)
    try:
        for s in strokes:
            ctx.brush([s], 5)
        assert ctx.edit_stats()[1] > 0
        ctx.copy(first, 5)
        _assert_levels(ctx, ws_mid, ws_mid, 5, "after the first copy")
        assert ctx.compact()[0] > 0
        ctx.copy(second, 5)
        _assert_levels(ctx, ws_b, ws_b, 5, "after the compaction and the second copy")
        _check_world(ctx, ws_b, _frames(ws_a)[1:3], "brush, copy, compact, copy")
        _check_picks(ctx, solid, colour, np.random.default_rng(8), 4096, "after the second copy")
    finally:
        ctx.close()
        ws_mid.close()
        ws_b.close()


def test_rejected_copies_leave_the_world_alone(world_a):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    try:
        good = _placement((10, 0, 10), (20, 30, 20), (50, 0, 50), 1, FILL, 1)
        bad_cases = [
            (dict(good, op=4), "bad op"), (dict(good, op=-1), "bad op"), (dict(good, move=2), "move"), (dict(good, transform=16), "transform bits"),
            (dict(good, srcMax=[10, 30, 20]), "empty"), (dict(good, srcMin=[0, -1, 0]), "empty or outside"),
            (dict(good, srcMax=[129, 30, 20]), "outside the world"), (dict(good, srcMax=[20, 65, 20]), "outside the world"),
            (dict(good, dst=[0, 0, (1 << 30) + 1]), "2\\^30"), (dict(good, dst=[-(1 << 30) - 1, 0, 0]), "2\\^30"),
        ]
        for bad, match in bad_cases:
            with pytest.raises(gpu.CvxError, match=match):
                ctx.copy([good, bad, good], 5)
        with pytest.raises(gpu.CvxError, match="levelCount"):
            ctx.copy([good], 6)
        with pytest.raises(gpu.CvxError, match="levelCount"):
            ctx.copy([good], -1)
        with pytest.raises(gpu.CvxError, match="placementCount"):
            ctx.copy([good] * (gpu.COPY_MAX_PLACEMENTS + 1), 5)
        with pytest.raises(gpu.CvxError, match="placementCount"):
            ctx.copy([], 5)
        assert ctx.copy([_placement((0, 0, 0), (8, 8, 8), (-20, 0, 0))], 5) == 0.0  # the destination outside the world: nothing to do
        _assert_levels(ctx, ws_a, ws_a, 5, "after the rejected copies")
        assert ctx.edit_stats()[1:] == (0, 0)
    finally:
        ctx.close()


def test_a_copy_over_the_format_limits_is_rejected_whole():
    """A placement in the middle of the list stacks a 20000-voxel column on top of itself into a run of 32768 voxels (RLEColumn keeps lengths in
    shorts): CVX_ERR_CAPACITY, and neither the placements before it nor the ones after it change the world."""
    dims = (32, 32768, 32)
    xs, zs = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    xs, zs = xs.ravel(), zs.ravel()
    ys = (xs * 7 + zs * 3) % 50
    tall = np.arange(20000)
    x = np.concatenate([xs, np.full(tall.size, 3)])
    y = np.concatenate([ys, tall])
    z = np.concatenate([zs, np.full(tall.size, 3)])
    keep = ~((x == 3) & (z == 3) & (y < 50) & (np.arange(x.size) < xs.size))
    x, y, z = x[keep], y[keep], z[keep]
    ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), _colour(x, y, z), threads=4)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        before = [ctx.read_level(k) for k in range(6)]
        placements = [_placement((10, 0, 10), (20, 40, 20), (0, 0, 20), 1, REPLACE, 1),
                      _placement((3, 0, 3), (4, 20000, 4), (3, 12768, 3), 8, FILL),
                      _placement((0, 0, 0), (4, 60, 4), (20, 0, 20), 0, FILL)]
        with pytest.raises(gpu.CvxError, match="32767"):
            ctx.copy(placements, 5)
        assert [ctx.read_level(k) for k in range(6)] == before
        assert ctx.edit_stats()[1:] == (0, 0)
        placements[1]["dst"] = [3, 12767, 3]  # one voxel lower: a run of 32767 fits
        ctx.copy(placements, 5)
        blob, _ = ctx.read_region(0, 3, 3, 1, 1)
        header = np.frombuffer(blob[:12], dtype=np.uint32)
        assert (header[1] & 0xFFFF, header[1] >> 16, header[2]) == (2, 0, 32767)
    finally:
        ctx.close()
        ws.close()
