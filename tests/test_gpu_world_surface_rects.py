"""GPU: the exposed faces of the device-resident world merged into rectangles (cvx_world_surface_rects, cvx_world_surface_rects_device).

Every case is called twice with identical bytes and checked four ways: the bytes equal those of the dense model of tests/surfacerectsmodel.py;
the rectangles' unit faces are, as exact multisets, the unit faces of the quads cvx_world_surface returns from the same context for the same call
(no model in that); no two rectangles of one face, plane and colour share a whole edge; and the summary.  The shapes at which the kernels can go
wrong are constructed: rectangles across wave, workgroup and scan-chunk boundaries, a chain of 1024 strips beside noise, rows that must not
stack, a box that cuts a floor, a column stored as two touching runs inside a uniform wall, before and after a compaction; the capacity in both
variants; rejected calls, and the world after the call."""
import numpy as np
import pytest
import torch

import surfacerectsmodel as model
from cpuvox_amd import gpu
from test_gpu_world_brush import _box, _brushed
from test_gpu_world_edit import DIMS
from test_gpu_world_pieces import built  # noqa: F401  (the fixture)
from test_gpu_world_surface import _built_world, _context
from test_world_brush_cpu import _pick_world
from test_world_cavities_cpu import NOISE_DIMS
from test_world_surface_rects_cpu import SLAB_SIZES, check_properties, l_floor, rows, slab_sizes, slab_world

pytestmark = pytest.mark.gpu

FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE
IGNORE = gpu.SURFACE_IGNORE_COLOUR
BLOCK_PAIRS = 256    # (column, face) pairs per workgroup of the kernels (cvx_surface_rects.hip, kThreads)
SCAN_CHUNK = 4096    # entries per workgroup of the prefix scans (cvx_downsample.h, CVX_SCAN_CHUNK)
SENTINEL = 0x5A5A5A5A
SLAB_DIMS = (256, 32, 128)  # the CPU test's slab world, 32 high: a context takes a world with all six LODs, and five halvings of 16 leave nothing


_MODEL = {}


def _model(solid, colour, box_min, box_max, solid_outside, flags):
    """model.rects, computed once per world and call (the arrays are kept with the result, so their ids stay theirs)."""
    key = (id(solid), id(colour), tuple(int(v) for v in box_min), tuple(int(v) for v in box_max), solid_outside, flags)
    if key not in _MODEL:
        _MODEL[key] = (model.rects(solid, colour, box_min, box_max, solid_outside, flags), solid, colour)
    return _MODEL[key][0]


def _rects(ctx, solid, colour, box_min, box_max, solid_outside=0x04, flags=0, label=""):
    """The call twice (identical bytes) against the model, against cvx_world_surface's own quads, and the whole-edge property."""
    want, want_summary = _model(solid, colour, box_min, box_max, solid_outside, flags)
    got, summary, ms = ctx.world_surface_rects(box_min, box_max, solid_outside, flags)
    again, summary_again, _ = ctx.world_surface_rects(box_min, box_max, solid_outside, flags)
    assert summary == want_summary, f"{label}: {summary} != {want_summary}"
    assert len(got) == len(want), label
    if got.tobytes() != want.tobytes():
        k = int(np.argmax(got != want))
        raise AssertionError(f"{label}: first difference at rectangle {k}: {got[k]} != {want[k]}")
    assert again.tobytes() == got.tobytes() and summary_again == summary, f"{label}: two calls differ"
    assert ms > 0.0, label
    quads, quad_summary, _ = ctx.world_surface(box_min, box_max, solid_outside, flags)
    assert (summary["strips"], summary["unitFaces"]) == (quad_summary["quads"], quad_summary["unitFaces"]), label
    lo, hi = np.maximum(np.array(box_min), 0), np.minimum(np.array(box_max), np.array(solid.shape))
    check_properties(got, summary, quads, flags, (lo, hi), label)
    return got, summary


def _rects_device(ctx, solid, colour, box_min, box_max, solid_outside, flags, capacity, label=""):
    """The device variant into a sentinel-filled buffer with one guard record behind the capacity."""
    want, want_summary = _model(solid, colour, box_min, box_max, solid_outside, flags)
    buffer = torch.full((capacity + 1, 8), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    summary, ms = ctx.world_surface_rects_device(box_min, box_max, buffer.data_ptr(), capacity, solid_outside, flags)
    torch.cuda.synchronize()
    raw = buffer.cpu().numpy()
    assert summary == want_summary and ms > 0.0, label
    listed = min(capacity, len(want))
    assert raw[:listed].tobytes() == want[:listed].tobytes(), label
    assert (raw[listed:].view(np.uint32) == SENTINEL).all(), f"{label}: something was written behind entry {listed}"
    return listed


def _few_colours(solid, seed, colours=3):
    rng = np.random.default_rng(seed)
    return np.where(solid, 0xFF000040 + rng.integers(0, colours, solid.shape), 0).astype(np.uint32)


# ---- whole worlds --------------------------------------------------------------------------------------------------------------------------------

def _checked_world(ctx, solid, colour, dims):
    merged = 0
    for flags in (0, IGNORE):
        for solid_outside in (0x04, 0, 0x3F):
            _, summary = _rects(ctx, solid, colour, (0, 0, 0), dims, solid_outside, flags, label=f"whole world, outside 0x{solid_outside:02x}, flags {flags}")
            merged += summary["strips"] - summary["rects"]
    _rects(ctx, solid, colour, (3, 2, 5), (dims[0] - 4, dims[1] - 3, dims[2] - 2), 0x04, 0, label="inner box")
    _rects(ctx, solid, colour, (3, 2, 5), (dims[0] - 4, dims[1] - 3, dims[2] - 2), 0x3B, IGNORE, label="inner box, collision mesh")
    _rects(ctx, solid, colour, (-5, -3, dims[2] // 2), (dims[0] // 2, dims[1] + 9, dims[2] + 4), 0x15, 0, label="partly outside the world")
    for flags in (0, IGNORE):
        _rects(ctx, solid, colour, (3, 0, 1), (4, dims[1], 2), 0x04, flags, label=f"one column, flags {flags}")
    _rects(ctx, solid, colour, (3, dims[1] // 4 - 2, 1), (4, dims[1] // 4 - 1, 2), 0x04, 0, label="one voxel")
    return merged


@pytest.mark.parametrize("dims", NOISE_DIMS)
def test_noise_worlds(dims):
    solid = np.random.default_rng(1).random(dims) < 0.7
    colour = _few_colours(solid, 2)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        assert _checked_world(ctx, solid, colour, dims) > 1000
    finally:
        ctx.close()
        ws.close()


def test_a_smooth_terrain():
    """A sine height field of 32 x 32 x 32 voxels coloured by height bands: floors that stack, walls that run along the slopes."""
    dims = (32, 32, 32)
    x, y, z = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    height = (14 + 6 * np.sin(x / 5.0) + 5 * np.cos(z / 7.0)).astype(np.int64)
    solid = y < height
    colour = np.where(solid, 0xFF204000 + (y // 4), 0).astype(np.uint32)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        assert _checked_world(ctx, solid, colour, dims) > 1000
    finally:
        ctx.close()
        ws.close()


def test_a_world_of_every_column_encoding():
    """Records with 1 .. 3 runs, run-list columns, both colour layouts, empty columns (every voxel its own colour: only IGNORE_COLOUR merges)."""
    dims = (32, 128, 32)
    solid, colour, ws = _pick_world(np.random.default_rng(3), dims, True)
    ctx = _context(ws)
    try:
        for flags in (0, IGNORE):
            _rects(ctx, solid, colour, (0, 0, 0), dims, 0x04, flags, label=f"whole world, flags {flags}")
            _rects(ctx, solid, colour, (2, 30, 3), (30, 100, 29), 0x3F, flags, label=f"inner box, flags {flags}")
    finally:
        ctx.close()
        ws.close()


# ---- the shapes at which the kernels can go wrong ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [(0, 0, 0), (54, 2, 55)])
def test_the_slab(offset):
    """130 x 3 x 70 voxels of one colour: 18 600 strips, 6 rectangles.  Where the CPU test has it the slab spans x = 64 and 128 and z = 64; moved, it
    starts at x = 64, where a workgroup's columns begin, spans x = 128 and z = 64 and ends at the world's face z = 128: the columns of a
    rectangle lie in several waves, workgroups and scan chunks, and no boundary may show."""
    solid, colour, (lo, hi) = slab_world(offset, SLAB_DIMS)
    assert all(hi[a] <= SLAB_DIMS[a] for a in range(3))
    ws = _built_world(SLAB_DIMS, solid, colour)
    ctx = _context(ws)
    try:
        for flags in (IGNORE, 0):
            rects, summary = _rects(ctx, solid, colour, (0, 0, 0), SLAB_DIMS, 0, flags, label=f"the slab at {lo}, flags {flags}")
            assert summary["rects"] == 6 and summary["rectsPerFace"] == [1] * 6 and summary["strips"] == 18600
            assert slab_sizes(rects) == SLAB_SIZES
        assert _rects_device(ctx, solid, colour, (0, 0, 0), SLAB_DIMS, 0, IGNORE, 8, label="device") == 6
    finally:
        ctx.close()
        ws.close()


def test_pair_counts_around_the_workgroup_and_the_scan_chunk_and_a_chain_of_1024():
    """A thin world, 2 x 32 x 1024, of noise in four colours with one solid layer of a colour of its own across all 1024 columns of z: its side
    faces are chains of 1024 strips, each walked by one thread, beside the noise.  Boxes of 1 x dimY x k columns whose 6 k pairs end less than a
    column below and above a workgroup (256) and a scan chunk (4096), and the whole world: three chunks."""
    dims = (2, 32, 1024)
    rng = np.random.default_rng(11)
    solid = rng.random(dims) < 0.6
    solid[:, 16, :] = True
    x, y, z = np.nonzero(solid)
    colour = np.zeros(dims, dtype=np.uint32)
    colour[x, y, z] = (0xFF000000 | ((x * 7 + y // 3 + z * 5) % 4)).astype(np.uint32)
    colour[:, 16, :] = 0xFFABCDEF
    sizes = sorted({edge // 6 + d for edge in (BLOCK_PAIRS, 2 * BLOCK_PAIRS, SCAN_CHUNK) for d in (-1, 0, 1)} | {1, 2})
    assert {42, 43, 682, 683} <= set(sizes)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        for k in sizes:
            rects, _ = _rects(ctx, solid, colour, (1, 0, 7), (2, 32, 7 + k), 0x04, 0, label=f"1 x 32 x {k} columns")
            layer = rects[(rects["argb"] == 0xFFABCDEF) & (rects["face"] == 1)]
            assert layer["size"].tolist() == [[1, 1, k]] and layer["voxel"].tolist() == [[1, 16, 7]]
            _rects(ctx, solid, colour, (0, 3, 7), (1, 29, 7 + k), 0x3F, IGNORE, label=f"1 x 26 x {k} columns, collision mesh")
        for flags in (0, IGNORE):
            rects, _ = _rects(ctx, solid, colour, (0, 0, 0), dims, 0, flags, label=f"three scan chunks, flags {flags}")
            if not flags:
                layer = rects[(rects["argb"] == 0xFFABCDEF) & (rects["face"] < 2)]
                assert layer["size"].tolist() == [[1, 1, 1024]] * 2 and layer["voxel"].tolist() == [[0, 16, 0], [1, 16, 0]]
        _rects_device(ctx, solid, colour, (0, 0, 0), dims, 0, 0, 5000, label="device, three scan chunks")
    finally:
        ctx.close()
        ws.close()


def test_rows_that_must_not_stack():
    """Two floors at one height that meet in an L: the rows of the two parts start at the same x and have different lengths.  The rule gives two
    rectangles per horizontal face; the model says which part takes the rows they could share.  Then rows of one length that start at
    different x, a floor sheared by one voxel per row: nothing stacks."""
    dims, solid, colour = l_floor()
    sheared = np.zeros(dims, dtype=bool)
    for k in range(8):
        sheared[3 + k:13 + k, 5, 4 + k] = True
    the_l = [((4, 3, 2), (20, 1, 8)), ((4, 3, 10), (8, 1, 12))]
    rows_alone = [((3 + k, 5, 4 + k), (10, 1, 1)) for k in range(8)]
    for name, solid, colour, want in (("the L", solid, colour, the_l), ("the sheared floor", sheared, np.where(sheared, 0xFFA0A0A0, 0).astype(np.uint32), rows_alone)):
        ws = _built_world(dims, solid, colour)
        ctx = _context(ws)
        try:
            for flags in (0, IGNORE):
                rects, _ = _rects(ctx, solid, colour, (0, 0, 0), dims, 0, flags, label=f"{name}, flags {flags}")
                for face in (2, 3):
                    part = rects[rects["face"] == face]
                    assert sorted(zip(map(tuple, part["voxel"].tolist()), map(tuple, part["size"].tolist()))) == want, (name, face)
        finally:
            ctx.close()
            ws.close()


def test_a_box_that_cuts_a_floor_in_two():
    solid, colour, _ = slab_world(dims=SLAB_DIMS)
    ws = _built_world(SLAB_DIMS, solid, colour)
    ctx = _context(ws)
    try:
        whole, _ = _rects(ctx, solid, colour, (0, 0, 0), SLAB_DIMS, 0x04, 0, label="whole")
        for cut_axis, cut in ((0, 77), (2, 64), (1, 6)):
            left_max, right_min = list(SLAB_DIMS), [0, 0, 0]
            left_max[cut_axis] = right_min[cut_axis] = cut
            left, _ = _rects(ctx, solid, colour, (0, 0, 0), left_max, 0x04, 0, label=f"below {cut} on axis {cut_axis}")
            right, _ = _rects(ctx, solid, colour, right_min, SLAB_DIMS, 0x04, 0, label=f"from {cut} on axis {cut_axis}")
            assert rows(model.unit_faces(np.concatenate([left, right]))) == rows(model.unit_faces(whole))
            assert (left["voxel"][:, cut_axis] + left["size"][:, cut_axis] <= cut).all() and (right["voxel"][:, cut_axis] >= cut).all()
            assert len(left) == 5 and len(right) == 5  # the cut faces are not exposed: the slab goes on across the seam
    finally:
        ctx.close()
        ws.close()


# ---- after edits, and the world after the call -------------------------------------------------------------------------------------------------

WALL = 0xFF808080
SCENE = [_box(FILL, (20, 10, 20), (60, 30, 24), WALL)]  # a wall of one colour, 40 x 20 x 4, above the floor
AROUND = ((10, 2, 10), (70, 40, 40))


def _wall_faces(rects):
    return {int(r["face"]): (tuple(int(v) for v in r["voxel"]), tuple(int(v) for v in r["size"])) for r in rects if r["argb"] == WALL}


def test_a_foreign_column_inside_a_uniform_wall(built):
    """A carve into the wall and a fill of the same voxels with the wall's colour: the edited columns hold their span as the brush left it, in
    runs that touch.  The wall is still one rectangle per face, before and after the compaction."""
    ctx, solid, colour = built(SCENE)
    want = {0: ((20, 10, 20), (1, 20, 4)), 1: ((59, 10, 20), (1, 20, 4)), 2: ((20, 10, 20), (40, 1, 4)), 3: ((20, 29, 20), (40, 1, 4)),
            4: ((20, 10, 20), (40, 20, 1)), 5: ((20, 10, 23), (40, 20, 1))}
    rects, _ = _rects(ctx, solid, colour, *AROUND, label="the wall")
    assert _wall_faces(rects) == want and len(rects) == 6
    strokes = [_box(CARVE, (30, 15, 20), (33, 22, 22)), _box(FILL, (30, 15, 20), (33, 22, 22), WALL), _box(CARVE, (45, 10, 22), (46, 18, 24)),
               _box(FILL, (45, 10, 22), (46, 18, 24), WALL)]
    for stroke in strokes:
        ctx.brush([stroke], 5)
        solid, colour = _brushed(solid, colour, [stroke])
    assert ctx.edit_stats()[1] > 0, "the edits left nothing behind: the compaction would move nothing"
    for flags in (0, IGNORE):
        rects, _ = _rects(ctx, solid, colour, *AROUND, 0x04, flags, label=f"after the carve and the fill, flags {flags}")
        assert _wall_faces(rects) == want and len(rects) == 6
    ctx.compact()
    for flags in (0, IGNORE):
        rects, _ = _rects(ctx, solid, colour, *AROUND, 0x04, flags, label=f"after the compaction, flags {flags}")
        assert _wall_faces(rects) == want and len(rects) == 6
    _rects(ctx, solid, colour, (0, 0, 0), DIMS, 0x04, IGNORE, label="after the compaction, whole world")
    assert _rects_device(ctx, solid, colour, *AROUND, 0x04, 0, 100, label="device, after the compaction") == 6


def test_capacity(built):
    ctx, solid, colour = built(SCENE + [_box(FILL, (70, 1, 70), (74, 50, 74), 0xFF2040C0), _box(CARVE, (30, 12, 18), (40, 20, 30))])
    box = ((10, 0, 10), (90, 64, 90))
    want, want_summary = _model(solid, colour, *box, 0x04, 0)
    total = len(want)
    assert total > 40
    listed, summary, _ = ctx.world_surface_rects(*box, 0x04, 0, capacity=0)
    assert len(listed) == 0 and summary == want_summary
    for capacity in (1, total // 2, total, total + 5):
        listed, summary, _ = ctx.world_surface_rects(*box, 0x04, 0, capacity=capacity)
        assert summary == want_summary and listed.tobytes() == want[:capacity].tobytes(), capacity
        assert _rects_device(ctx, solid, colour, *box, 0x04, 0, capacity, label=f"device, capacity {capacity}") == min(capacity, total)
    _rects_device(ctx, solid, colour, (0, 0, 0), (8, 64, 8), 0x3F, IGNORE, 4, label="device, nothing exposed but the floor's top")
    _rects_device(ctx, solid, colour, (0, 1, 0), (8, 64, 8), 0, 0, 4, label="device, no solid voxel in the box")


def test_rejected_calls_and_the_world_after_the_calls(built):
    ctx, solid, colour = built(SCENE)
    before = [ctx.read_level(k) for k in range(6)]
    stats = ctx.edit_stats()
    bad = [(dict(box_min=(0, 0, 0), box_max=(0, 8, 8)), "empty"), (dict(box_min=(9, 0, 0), box_max=(8, 8, 8)), "empty"),
           (dict(box_min=(0, 64, 0), box_max=(8, 70, 8)), "outside the world"), (dict(box_min=(-9, 0, 0), box_max=(0, 8, 8)), "outside the world"),
           (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), solid_outside=0x40), "solidOutside"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), solid_outside=-1), "solidOutside"),
           (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), flags=2), "flags"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), capacity=-1), "rectCapacity")]
    for kwargs, match in bad:
        with pytest.raises(gpu.CvxError, match=match):
            ctx.world_surface_rects(**kwargs)
    with pytest.raises(gpu.CvxError, match="rectCapacity"):
        ctx.world_surface_rects_device((0, 0, 0), (8, 8, 8), 0, 4)
    fresh = gpu.Context(0)
    try:
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.world_surface_rects((0, 0, 0), (8, 8, 8))
    finally:
        fresh.close()
    assert [ctx.read_level(k) for k in range(6)] == before and ctx.edit_stats() == stats, "a rejected call changed the arena"
    _rects(ctx, solid, colour, *AROUND, label="after the rejected calls")
    _rects(ctx, solid, colour, (0, 0, 0), DIMS, 0x3F, IGNORE, label="whole world")
    _rects_device(ctx, solid, colour, *AROUND, 0x04, 0, 3, label="device")
    assert [ctx.read_level(k) for k in range(6)] == before and ctx.edit_stats() == stats, "a call changed the arena"


def test_the_list_around_the_count_in_both_forms():
    """An 8 x 8 x 8 box of a 16 x 16 x 16 noise world, capacities 0 (no list), 1, found - 1, found and found + 1: the host and the device form
    give the same bytes, leave a list filled with a sentinel alone from min(found, capacity) on, and the summary is the same at every capacity."""
    dims, box = (16, 16, 16), ((4, 4, 4), (12, 12, 12))
    solid = np.random.default_rng(7).random(dims) < 0.5
    colour = _few_colours(solid, 8)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        want, want_summary = model.rects(solid, colour, *box, 0x04, 0)
        found = len(want)
        assert found > 2
        for capacity in (0, 1, found - 1, found, found + 1):
            listed = min(capacity, found)
            on_host = np.full((found + 2, 8), SENTINEL, dtype=np.uint32)
            on_device = torch.full((found + 2, 8), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            summary, _ = ctx._surface_rects(gpu.lib().cvx_world_surface_rects, *box, 0x04, 0, on_host.ctypes.data if capacity else None, capacity)
            device_summary, _ = ctx.world_surface_rects_device(*box, on_device.data_ptr() if capacity else 0, capacity, 0x04, 0)
            torch.cuda.synchronize()
            back = on_device.cpu().numpy().view(np.uint32)
            assert summary == want_summary and device_summary == want_summary, capacity
            assert on_host[:listed].tobytes() == want[:listed].tobytes() and back[:listed].tobytes() == want[:listed].tobytes(), capacity
            assert (on_host[listed:] == SENTINEL).all() and (back[listed:] == SENTINEL).all(), f"capacity {capacity}: written behind entry {listed}"
    finally:
        ctx.close()
        ws.close()
