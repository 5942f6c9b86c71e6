"""GPU: the exposed faces of the device-resident world as coloured quads (cvx_world_surface, cvx_world_surface_device).

Every call is made twice with identical bytes and compared byte for byte with the dense model of tests/surfacemodel.py (shifted comparisons on
the numpy volume the world was built from and the brush strokes were applied to): the summary as exact integers, the first `capacity` quads as
bytes.  The device variant writes into a buffer filled with a sentinel: what lies behind min(capacity, quads) must still be the sentinel.  The
shapes at which the kernels can go wrong -- pair counts around the workgroup and the scan chunk, a column of 128 quads per pair, the most faces
per voxel, nothing at all -- are constructed; after edits and a compaction the surface follows the model; the call leaves the world as it was."""
import numpy as np
import pytest
import torch

import surfacemodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _box, _brushed
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _frames
from test_gpu_world_pieces import built  # noqa: F401  (the fixture)
from test_world_brush_cpu import _pick_world
from test_world_cavities_cpu import NOISE_DIMS, noise_world
from test_world_surface_cpu import random_call, world_boxes

pytestmark = pytest.mark.gpu

FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE
IGNORE = gpu.SURFACE_IGNORE_COLOUR
BLOCK_PAIRS = 256    # (column, face) pairs per workgroup of the count and write kernels (cvx_surface.hip, kThreads)
SCAN_CHUNK = 4096    # entries per workgroup of the prefix scan (cvx_downsample.h, CVX_SCAN_CHUNK)
SENTINEL = 0x5A5A5A5A


def _surface(ctx, solid, colour, box_min, box_max, solid_outside=0x04, flags=0, capacity=None, label=""):
    """The call twice (identical bytes) against the model: the summary, and the first `capacity` quads byte for byte."""
    want, want_summary = surfacemodel.surface(solid, colour, box_min, box_max, solid_outside, flags)
    got, summary, ms = ctx.world_surface(box_min, box_max, solid_outside, flags, capacity)
    again, summary_again, _ = ctx.world_surface(box_min, box_max, solid_outside, flags, capacity)
    assert summary == want_summary, f"{label}: {summary} != {want_summary}"
    listed = len(want) if capacity is None else min(capacity, len(want))
    assert len(got) == listed, label
    if got.tobytes() != want[:listed].tobytes():
        k = int(np.argmax(got != want[:listed]))
        raise AssertionError(f"{label}: first difference at quad {k}: {got[k]} != {want[k]}")
    assert again.tobytes() == got.tobytes() and summary_again == summary, f"{label}: two calls differ"
    assert ms > 0.0, label
    return got, summary


def _surface_device(ctx, solid, colour, box_min, box_max, solid_outside, flags, capacity, label=""):
    """The device variant into a sentinel-filled buffer with one guard record behind the capacity."""
    want, want_summary = surfacemodel.surface(solid, colour, box_min, box_max, solid_outside, flags)
    buffer = torch.full((capacity + 1, 6), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    summary, ms = ctx.world_surface_device(box_min, box_max, buffer.data_ptr(), capacity, solid_outside, flags)
    torch.cuda.synchronize()
    raw = buffer.cpu().numpy()
    assert summary == want_summary and ms > 0.0, label
    listed = min(capacity, len(want))
    assert raw[:listed].tobytes() == want[:listed].tobytes(), label
    assert (raw[listed:].view(np.uint32) == SENTINEL).all(), f"{label}: something was written behind entry {listed}"


def _context(ws):
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    return ctx


def _checked_world(solid, colour, ws, dims, seed):
    ctx = _context(ws)
    try:
        for name, (box_min, box_max, solid_outside, flags) in world_boxes(dims).items():
            _surface(ctx, solid, colour, box_min, box_max, solid_outside, flags, label=name)
        rng = np.random.default_rng(seed)
        for k in range(40):
            box_min, box_max, solid_outside, flags = random_call(rng, dims)
            capacity = [0, 3, None][int(rng.integers(0, 3))]
            _surface(ctx, solid, colour, box_min, box_max, solid_outside, flags, capacity, label=f"random call {k}")
        total = surfacemodel.surface(solid, colour, (0, 0, 0), dims, 0x04, 0)[1]["quads"]
        for capacity in (0, 3, total, total + 5):
            _surface(ctx, solid, colour, (0, 0, 0), dims, 0x04, 0, capacity, label=f"capacity {capacity}")
            _surface_device(ctx, solid, colour, (0, 0, 0), dims, 0x04, IGNORE, max(capacity, 1), label=f"device, capacity {capacity}")
        _surface_device(ctx, solid, colour, (3, 2, 5), (dims[0] - 4, dims[1] - 3, dims[2] - 2), 0x3B, 0, 3, label="device, inner box")
    finally:
        ctx.close()


# ---- whole worlds --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", NOISE_DIMS)
def test_noise_worlds(dims):
    solid, colour, ws = noise_world(dims)
    try:
        _checked_world(solid, colour, ws, dims, dims[0] + 200)
    finally:
        ws.close()


@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((32, 128, 32), True, 3)])
def test_terrain_worlds(dims, sparse, seed):
    """Records with 1 .. 3 runs, run-list columns, both colour layouts, empty columns."""
    solid, colour, ws = _pick_world(np.random.default_rng(seed), dims, sparse)
    try:
        _checked_world(solid, colour, ws, dims, seed + 300)
    finally:
        ws.close()


# ---- the shapes at which the kernels can go wrong ------------------------------------------------------------------------------------------------

def _built_world(dims, solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def test_pair_counts_around_the_workgroup_and_the_scan_chunk():
    """A thin world, 2 x 32 x 1024: boxes of 1 x dimY x k columns whose 6 k pairs end less than a column below and above a workgroup (256) and
    a scan chunk (4096); the scan takes the pairs and one more entry, so the k whose 6 k + 1 entries straddle the chunk are there too; and boxes
    of more than one chunk in one row and in both."""
    dims = (2, 32, 1024)
    rng = np.random.default_rng(11)
    solid = rng.random(dims) < 0.6
    colour = np.zeros(dims, dtype=np.uint32)
    x, y, z = np.nonzero(solid)
    colour[x, y, z] = (0xFF000000 | ((x * 7 + y // 3 + z * 5) % 4)).astype(np.uint32)  # few colours: quads longer than a voxel
    sizes = sorted({edge // 6 + d for edge in (BLOCK_PAIRS, 2 * BLOCK_PAIRS, SCAN_CHUNK) for d in (-1, 0, 1)} | {1, 2, 1024})
    assert {42, 43, 682, 683} <= set(sizes)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        for k in sizes:
            z0 = 0 if k == 1024 else 7
            _surface(ctx, solid, colour, (1, 0, z0), (2, 32, z0 + k), 0x04, 0, label=f"1 x 32 x {k} columns")
            _surface(ctx, solid, colour, (0, 3, z0), (1, 29, z0 + k), 0x3F, IGNORE, label=f"1 x 26 x {k} columns, collision mesh")
        _surface(ctx, solid, colour, (0, 0, 0), dims, 0x04, 0, label="three scan chunks")
        _surface_device(ctx, solid, colour, (0, 0, 0), dims, 0, 0, 5000, label="device, three scan chunks")
    finally:
        ctx.close()
        ws.close()


def test_pillar_checkerboard_empty_box_and_one_voxel():
    dims = (32, 128, 32)
    solid = np.zeros(dims, dtype=bool)
    colour = np.zeros(dims, dtype=np.uint32)
    solid[5, :, 9] = True                                          # a 1 x 128 x 1 pillar of alternating colours
    colour[5, :, 9] = np.where(np.arange(128) % 2 == 0, 0xFF0000FF, 0xFF00FF00).astype(np.uint32)
    x, y, z = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    board = (x + y + z) % 2 == 0                                   # an 8 x 8 x 8 checkerboard: six exposed faces per voxel
    solid[16:24, 40:48, 16:24] = board
    colour[16:24, 40:48, 16:24] = np.where(board, 0xFF808080, 0).astype(np.uint32)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        pillar = ((5, 0, 9), (6, 128, 10))
        quads, summary = _surface(ctx, solid, colour, *pillar, 0x04, 0, label="pillar")
        assert summary["quadsPerFace"] == [128, 128, 0, 1, 128, 128] and summary["unitFaces"] == 4 * 128 + 1
        quads, summary = _surface(ctx, solid, colour, *pillar, 0x04, IGNORE, label="pillar, collision mesh")
        assert summary["quadsPerFace"] == [1, 1, 0, 1, 1, 1] and summary["unitFaces"] == 4 * 128 + 1
        assert quads["length"].tolist() == [128, 128, 1, 128, 128] and (quads["argb"] == 0xFF00FF00).all()  # the top voxel's colour (y = 127)
        _, summary = _surface(ctx, solid, colour, (5, 0, 9), (6, 128, 10), 0, 0, label="pillar in air")
        assert summary["quadsPerFace"][2] == 1
        _, summary = _surface(ctx, solid, colour, (16, 40, 16), (24, 48, 24), 0x04, 0, label="checkerboard")
        assert summary["quads"] == summary["unitFaces"] == 6 * 256 and summary["quadsPerFace"] == [256] * 6
        _surface(ctx, solid, colour, (14, 38, 14), (26, 50, 26), 0x04, IGNORE, label="checkerboard, collision mesh")
        quads, summary = _surface(ctx, solid, colour, (0, 0, 0), (4, 128, 32), 0x3F, 0, label="no solid voxel in the box")
        assert summary == {"quads": 0, "unitFaces": 0, "quadsPerFace": [0] * 6} and len(quads) == 0
        _surface_device(ctx, solid, colour, (0, 0, 0), (4, 128, 32), 0, 0, 4, label="device, no solid voxel in the box")
        quads, summary = _surface(ctx, solid, colour, (5, 77, 9), (6, 78, 10), 0x04, 0, label="one voxel of the pillar")
        assert quads["face"].tolist() == [0, 1, 4, 5] and (quads["voxel"] == (5, 77, 9)).all()
        quads, _ = _surface(ctx, solid, colour, (5, 127, 9), (6, 128, 10), 0x04, 0, label="the pillar's top voxel")
        assert quads["face"].tolist() == [0, 1, 3, 4, 5]
        _, summary = _surface(ctx, solid, colour, (7, 77, 9), (8, 78, 10), 0x04, 0, label="one voxel of air")
        assert summary["quads"] == 0
    finally:
        ctx.close()
        ws.close()


def test_boxes_on_the_six_world_faces():
    """A solid block that fills the world: only the world's boundary is exposed, face by face as solidOutside says."""
    dims = (32, 32, 32)
    solid = np.ones(dims, dtype=bool)
    colour = np.full(dims, 0xFF336699, dtype=np.uint32)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        for f in range(6):
            a, up = f // 2, f % 2
            lo, hi = [4, 4, 4], [28, 28, 28]
            lo[a], hi[a] = (24, 40) if up else (-8, 8)  # the box touches world face f only
            _, summary = _surface(ctx, solid, colour, lo, hi, 0x3F & ~(1 << f), 0, label=f"face {f} open")
            want = [0] * 6
            want[f] = 24 * 24 if a == 1 else 24
            assert summary["quadsPerFace"] == want and summary["unitFaces"] == 24 * 24, (f, summary)
            _, summary = _surface(ctx, solid, colour, lo, hi, 1 << f, 0, label=f"face {f} solid outside")
            assert summary["quads"] == 0, (f, summary)
        _, summary = _surface(ctx, solid, colour, (0, 0, 0), dims, 0, IGNORE, label="the whole block in air")
        assert summary["quadsPerFace"] == [32, 32, 1024, 1024, 32, 32] and summary["unitFaces"] == 6 * 32 * 32
    finally:
        ctx.close()
        ws.close()


# ---- after edits, and the world after the call -------------------------------------------------------------------------------------------------

SCENE = [_box(FILL, (20, 1, 20), (60, 30, 60), 0xFF808080), _box(CARVE, (30, 10, 30), (40, 20, 40)), _box(FILL, (70, 1, 70), (74, 50, 74), 0xFF2040C0)]
AROUND = ((10, 0, 10), (90, 64, 90))


def test_after_a_carve_a_fill_and_a_compaction(built):
    ctx, solid, colour = built(SCENE)
    _surface(ctx, solid, colour, *AROUND, label="the scene")
    _surface(ctx, solid, colour, (0, 0, 0), DIMS, 0x04, IGNORE, label="the scene, whole world")
    steps = [("carve", [_box(CARVE, (25, 5, 15), (35, 40, 45))]),
             ("fill with a second colour", [_box(FILL, (28, 12, 28), (50, 36, 33), 0xFFEE2211), {"op": FILL, "shape": gpu.SHAPE_SPHERE, "a": (72, 55, 72), "radius": 6, "argb": 0xFFEE2211}])]
    for name, strokes in steps:
        ctx.brush(strokes, 5)
        solid, colour = _brushed(solid, colour, strokes)
        _surface(ctx, solid, colour, *AROUND, label=f"after the {name}")
        _surface(ctx, solid, colour, *AROUND, 0x04, IGNORE, label=f"after the {name}, collision mesh")
    assert ctx.edit_stats()[1] > 0, "the edits left nothing behind: the compaction would move nothing"
    ctx.compact()
    _surface(ctx, solid, colour, *AROUND, label="after the compaction")
    _surface(ctx, solid, colour, (0, 0, 0), DIMS, 0, 0, label="after the compaction, whole world")
    _surface_device(ctx, solid, colour, *AROUND, 0x04, 0, 1000, label="device, after the compaction")


def test_the_call_leaves_the_world_as_it_was(built):
    ctx, solid, colour = built(SCENE)
    x, y, z = np.nonzero(solid)
    ws = host.WorldSet.from_voxels(DIMS, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)
    try:
        before = [ctx.read_level(k) for k in range(6)]
        stats = ctx.edit_stats()
        _, summary = _surface(ctx, solid, colour, (0, 0, 0), DIMS, label="whole world")
        assert summary["quads"] > 10000
        _surface(ctx, solid, colour, *AROUND, 0x3F, IGNORE, capacity=3, label="a box")
        _surface_device(ctx, solid, colour, *AROUND, 0x04, 0, 64, label="device")
        assert [ctx.read_level(k) for k in range(6)] == before and ctx.edit_stats() == stats, "a surface call changed the arena"
        _assert_levels(ctx, ws, ws, 5, "after the surface calls")
        visited = _check_world(ctx, ws, _frames(ws)[:2], "after the surface calls")
        assert visited[0] > 0
    finally:
        ws.close()


def test_rejected_calls(built):
    ctx, solid, colour = built(SCENE)
    bad = [(dict(box_min=(0, 0, 0), box_max=(0, 8, 8)), "empty"), (dict(box_min=(9, 0, 0), box_max=(8, 8, 8)), "empty"),
           (dict(box_min=(0, 64, 0), box_max=(8, 70, 8)), "outside the world"), (dict(box_min=(-9, 0, 0), box_max=(0, 8, 8)), "outside the world"),
           (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), solid_outside=0x40), "solidOutside"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), solid_outside=-1), "solidOutside"),
           (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), flags=2), "flags"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), capacity=-1), "quadCapacity")]
    for kwargs, match in bad:
        with pytest.raises(gpu.CvxError, match=match):
            ctx.world_surface(**kwargs)
    with pytest.raises(gpu.CvxError, match="quadCapacity"):
        ctx.world_surface_device((0, 0, 0), (8, 8, 8), 0, 4)
    fresh = gpu.Context(0)
    try:
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.world_surface((0, 0, 0), (8, 8, 8))
    finally:
        fresh.close()
    _surface(ctx, solid, colour, *AROUND, label="after the rejected calls")


def test_the_list_around_the_count_in_both_forms():
    """An 8 x 8 x 8 box of a 16 x 16 x 16 noise world, capacities 0 (no list), 1, found - 1, found and found + 1: the host and the device form
    give the same bytes, leave a list filled with a sentinel alone from min(found, capacity) on, and the summary is the same at every capacity."""
    dims, box = (16, 16, 16), ((4, 4, 4), (12, 12, 12))
    solid = np.random.default_rng(7).random(dims) < 0.5
    colour = np.where(solid, 0xFF204060, 0).astype(np.uint32)
    ws = _built_world(dims, solid, colour)
    ctx = _context(ws)
    try:
        want, want_summary = surfacemodel.surface(solid, colour, *box, 0x04, 0)
        found = len(want)
        assert found > 2
        for capacity in (0, 1, found - 1, found, found + 1):
            listed = min(capacity, found)
            on_host = np.full((found + 2, 6), SENTINEL, dtype=np.uint32)
            on_device = torch.full((found + 2, 6), SENTINEL, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            summary, _ = ctx._surface(gpu.lib().cvx_world_surface, *box, 0x04, 0, on_host.ctypes.data if capacity else None, capacity)
            device_summary, _ = ctx.world_surface_device(*box, on_device.data_ptr() if capacity else 0, capacity, 0x04, 0)
            torch.cuda.synchronize()
            back = on_device.cpu().numpy().view(np.uint32)
            assert summary == want_summary and device_summary == want_summary, capacity
            assert on_host[:listed].tobytes() == want[:listed].tobytes() and back[:listed].tobytes() == want[:listed].tobytes(), capacity
            assert (on_host[listed:] == SENTINEL).all() and (back[listed:] == SENTINEL).all(), f"capacity {capacity}: written behind entry {listed}"
    finally:
        ctx.close()
        ws.close()
