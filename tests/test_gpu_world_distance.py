"""GPU: exact squared-distance fields of boxes of the device-resident world (cvx_world_distance[_device]).

Every field is compared, element for element, with the dense numpy model of tests/distancemodel.py, which knows nothing about runs: it pads the
box by R according to the outside rule and takes a windowed min-plus along each axis.  The worlds are those of tests/test_gpu_world_dense.py:
the 128 x 64 x 128 terrain and the 32 x 256 x 32 tall world.  A voxel's result does not depend on the box, so the model's field of one box
that covers all the boxes of a test is computed once and sliced.  Every case asserts from the model that its input has the property it is
named for before it calls the device."""
import functools

import numpy as np
import pytest

import distancemodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _brushed, _dense, _world
from test_gpu_world_dense import TALL, _any_world, _tall_solid
from test_gpu_world_edit import DIMS, _context, _terrain
from test_world_dense_cpu import read_boxes

pytestmark = pytest.mark.gpu

FAR = gpu.DISTANCE_FAR
TO_SOLID, TO_AIR, SIGNED = gpu.DISTANCE_TO_SOLID, gpu.DISTANCE_TO_AIR, gpu.DISTANCE_SIGNED
MODES = {"to solid": TO_SOLID, "to air": TO_AIR, "signed": SIGNED}
GROUND = gpu.SURFACE_OUTSIDE_DEFAULT


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    colour = _dense(solid)
    return solid, colour, _world(solid, colour)


@pytest.fixture(scope="module")
def world_tall():
    solid = _tall_solid()
    colour = _dense(solid)
    return solid, colour, _any_world(TALL, solid, colour)


@pytest.fixture(scope="module")
def ctx_a(world_a):
    """A context of the terrain for the tests that only read."""
    ctx = _context(world_a[2])
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx_tall(world_tall):
    ctx = gpu.Context(0)
    ctx.upload_world(world_tall[2])
    yield ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def _reference(world, R, mode, outside, lo, hi):
    """The model's field of [lo, hi) of the terrain / the tall world, computed once and left alone."""
    solid = _terrain() if world == "terrain" else _tall_solid()
    out = distancemodel.field(solid, (lo, hi), R, mode, outside)
    out.setflags(write=False)
    return out


def _sliced(reference, ref_lo, lo, hi):
    """The box [lo, hi) out of a field that starts at ref_lo; both in (x, y, z), the field in (X, Z, Y)."""
    return reference[lo[0] - ref_lo[0]:hi[0] - ref_lo[0], lo[2] - ref_lo[2]:hi[2] - ref_lo[2], lo[1] - ref_lo[1]:hi[1] - ref_lo[1]]


def _same(got, want, label):
    assert got.shape == want.shape and got.dtype == np.int32, (label, got.shape, want.shape, got.dtype)
    bad = got != want
    assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()} (x, z, y): {got[bad][0]} for {want[bad][0]}"


# ---- 1. boxes -----------------------------------------------------------------------------------------------------------------------------------

def _check_boxes(ctx, world, dims, mode):
    boxes = read_boxes(dims)
    assert {b[1][1] - b[0][1] for b in boxes.values()} >= {1, 3, 63, 64, 65, 129} and all(b[0][1] % 64 for n, b in boxes.items() if n.startswith("height"))
    assert any(all(lo[a] < 0 and hi[a] > dims[a] for a in range(3)) for lo, hi in boxes.values()), "one box sticks out on six sides"
    assert any(lo[0] >= dims[0] for lo, _ in boxes.values()), "one box lies wholly outside"
    ref_lo = tuple(min(lo[a] for lo, _ in boxes.values()) for a in range(3))
    ref_hi = tuple(max(hi[a] for _, hi in boxes.values()) for a in range(3))
    reference = _reference(world, 8, mode, GROUND, ref_lo, ref_hi)
    kinds = set()
    for name, (lo, hi) in boxes.items():
        want = _sliced(reference, ref_lo, lo, hi)
        kinds |= {"zero"} if ((want < 0) if mode == SIGNED else (want == 0)).any() else set()  # (a signed field is negative there)
        kinds |= {"near"} if ((want != 0) & (abs(want) != FAR)).any() else set()
        kinds |= {"far"} if (abs(want) == FAR).any() else set()
        _same(ctx.distance(lo, hi, 8, mode), want, f"{name}, mode {mode}")
    assert kinds == {"zero", "near", "far"}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_boxes_equal_the_model(ctx_a, mode):
    _check_boxes(ctx_a, "terrain", DIMS, MODES[mode])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_boxes_equal_the_model_in_the_tall_world(ctx_tall, mode):
    _check_boxes(ctx_tall, "tall", TALL, MODES[mode])


# ---- 2. radii -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 2, 3, 20])
def test_radii_on_the_whole_terrain(ctx_a, R):
    want = _reference("terrain", R, TO_SOLID, GROUND, (0, 0, 0), DIMS)
    near = np.unique(want[want != FAR])
    squares = {k * k for k in range(R + 1)}
    if R >= 2:
        assert {2, 3} <= set(near.tolist()) and set(near.tolist()) - squares, "diagonal nearest voxels: values that are no squares"
    assert near.max() == R * R and len(near) == {1: 2, 2: 5, 3: 9, 20: 336}[R], (R, len(near))
    assert (want == FAR).any()
    _same(ctx_a.distance((0, 0, 0), DIMS, R), want, f"R {R}")


# ---- 3. the nearest solid voxel lies outside the box ---------------------------------------------------------------------------------------------

def test_nearest_solid_outside_the_box(ctx_a, world_a):
    solid = world_a[0]
    lo, hi = (40, 22, 40), (60, 32, 60)
    assert not solid[40:60, 22:32, 40:60].any(), "the box holds no solid voxel"
    want = _reference("terrain", 8, TO_SOLID, GROUND, lo, hi)
    assert want.size == 4000 and int((want != FAR).sum()) == 2188 and (want > 0).all()
    _same(ctx_a.distance(lo, hi, 8), want, "a box of air")


def test_the_ground_below_a_pit(world_a):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    try:
        pit = np.ones((16, 16, 40), dtype=bool)  # (X, Z, Y): the columns of [60, 76) x [60, 76) carved down to y = 0
        ctx.write_voxels((60, 0, 60), None, pit, gpu.BRUSH_CARVE)
        solid = solid_a.copy()
        solid[60:76, 0:40, 60:76] = False
        assert solid_a[60:76, 0, 60:76].all() and not solid[60:76, :, 60:76].any()
        lo, hi = (64, 0, 64), (72, 4, 72)
        with_ground = distancemodel.field(solid, (lo, hi), 8, TO_SOLID, GROUND)
        without = distancemodel.field(solid, (lo, hi), 8, TO_SOLID, 0)
        assert (with_ground[:, :, 0] == 1).all() and (with_ground[2:6, 2:6, 3] == 16).all(), "the nearest solid voxel is the ground below the world"
        assert (without[3:5, 3:5] >= 25).all() and (without != with_ground).any() and (without != FAR).any(), "without it, the pit's walls"
        _same(ctx.distance(lo, hi, 8, TO_SOLID, GROUND), with_ground, "solidOutside 0x04")
        _same(ctx.distance(lo, hi, 8, TO_SOLID, 0), without, "solidOutside 0")
    finally:
        ctx.close()


def test_the_world_edge_in_plus_x(ctx_a, world_a):
    solid = world_a[0]
    lo, hi = (DIMS[0] - 8, 48, 50), (DIMS[0] + 3, 58, 60)  # (more than 8 above the slabs)
    for mode in (TO_SOLID, SIGNED):
        wall = distancemodel.field(solid, (lo, hi), 8, mode, GROUND | 0x02)
        open_ = distancemodel.field(solid, (lo, hi), 8, mode, GROUND)
        inside = wall[:8]
        assert (inside[7] == 1).all() and (inside[0] == 64).all() and (abs(open_[:8]) == FAR).all(), "only the wall beyond +X is near"
        assert (wall[8:] <= 0).all() and (open_[8:] == FAR).all(), "beyond the face: solid, or air far from everything"
        _same(ctx_a.distance(lo, hi, 8, mode, GROUND | 0x02), wall, f"bit 1 set, mode {mode}")
        _same(ctx_a.distance(lo, hi, 8, mode, GROUND), open_, f"bit 1 clear, mode {mode}")


# ---- 4. the largest radius -----------------------------------------------------------------------------------------------------------------------

def _corner_world():
    """About a dozen solid voxels in one bottom corner of the tall world: (points, world set)."""
    rng = np.random.default_rng(17)
    points = np.stack([rng.integers(0, 10, 12), rng.integers(0, 2, 12), rng.integers(0, 10, 12)], axis=1)
    points[0] = (3, 0, 5)  # all in one bottom corner: the top of the world is some 254 voxels from the nearest
    points = np.unique(points, axis=0)
    assert 10 <= len(points) <= 12
    return points, host.WorldSet.from_voxels(TALL, points[:, 0].astype(np.int32), points[:, 1].astype(np.int32), points[:, 2].astype(np.int32),
                                             np.full(len(points), 0xFFCC8844, dtype=np.uint32), threads=2)


def test_radius_255_in_a_nearly_empty_world():
    points, ws = _corner_world()
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        box = ((0, 0, 0), TALL)
        sparse = distancemodel.sparse_field(points, box, 255)
        assert (sparse == 0).sum() == len(points)
        near = sparse[sparse != FAR]
        assert near.max() > 250 * 250 and near.size < sparse.size, "distances beyond 250 and voxels out of reach, both"
        _same(ctx.distance(*box, 255, TO_SOLID, 0), sparse, "solidOutside 0")
        ground = np.broadcast_to(((np.arange(TALL[1], dtype=np.int64) + 1) ** 2), sparse.shape)  # (y + 1)^2: the ground's voxel below
        want = np.minimum(sparse, np.where(ground <= 255 * 255, ground, FAR)).astype(np.int32)
        assert (want != sparse).any() and (want[:, :, 255] == sparse[:, :, 255]).all(), "the ground is nearer somewhere, and out of reach from y = 255"
        _same(ctx.distance(*box, 255, TO_SOLID, GROUND), want, "solidOutside 0x04")
    finally:
        ctx.close()
        ws.close()


def test_more_than_2_to_the_31_intermediate_elements():
    """One column 8300 voxels high at R = 255: the footprint grown by R holds 511 x 511 columns, 2 167 304 300 elements of the first intermediate
    array (4.3 GB), so element indices pass 2^31; the box, 8300 voxels, stays small.  Most of it lies below and above the world."""
    points, ws = _corner_world()
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        box = ((4, -4000, 4), (5, 4300, 5))
        assert 511 * 511 * (box[1][1] - box[0][1]) > 1 << 31
        want = distancemodel.sparse_field(points, box, 255)
        assert (want == FAR).sum() > 7000 and ((want != FAR) & (want > 0)).sum() > 400, "far below, near inside, far above"
        _same(ctx.distance(*box, 255, TO_SOLID, 0), want, "a column of 8300")
    finally:
        ctx.close()
        ws.close()


# ---- 5. tiling and determinism ------------------------------------------------------------------------------------------------------------------

def test_boxes_tile_and_calls_repeat(ctx_a):
    before = [ctx_a.read_level(lod) for lod in range(gpu.LOD_LEVELS)]
    cuts = [(0, 61, DIMS[0]), (0, 29, DIMS[1]), (0, 67, DIMS[2])]
    assert all(c[1] % 2 == 1 for c in cuts)
    for mode in (TO_SOLID, SIGNED):
        whole = ctx_a.distance((0, 0, 0), DIMS, 8, mode)
        tiles = [[[ctx_a.distance((cuts[0][i], cuts[1][j], cuts[2][k]), (cuts[0][i + 1], cuts[1][j + 1], cuts[2][k + 1]), 8, mode) for j in range(2)]
                  for k in range(2)] for i in range(2)]
        joined = np.concatenate([np.concatenate([np.concatenate(tiles[i][k], axis=2) for k in range(2)], axis=1) for i in range(2)], axis=0)
        _same(joined, whole, f"2 x 2 x 2 boxes, mode {mode}")
        assert ctx_a.distance((0, 0, 0), DIMS, 8, mode).tobytes() == whole.tobytes(), "the same call twice"
    assert [ctx_a.read_level(lod) for lod in range(gpu.LOD_LEVELS)] == before, "the calls only read the arena"


# ---- 6. the device variant ----------------------------------------------------------------------------------------------------------------------

def test_device_variant_writes_the_tensor_and_nothing_else(ctx_a):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    dev = torch.device("cuda", 0)
    lo, hi = (-3, 5, 90), (38, 70, 131)  # sticks out in -x, +y and +z
    shape = (hi[0] - lo[0], hi[2] - lo[2], hi[1] - lo[1])
    n, guard = shape[0] * shape[1] * shape[2], 4096
    for mode in MODES.values():
        flat = torch.full((n + guard,), -77, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ms = ctx_a.distance_device(lo, hi, 8, flat.data_ptr(), mode)
        assert ms > 0.0
        got = flat.cpu().numpy()  # (the call returned: the field is complete)
        assert (got[n:] == -77).all(), "the guard behind the tensor"
        want = ctx_a.distance(lo, hi, 8, mode)
        assert (want <= 0).any() and (abs(want) == FAR).any() and len(np.unique(want)) > 10, "solid, near and far voxels"
        _same(got[:n].reshape(shape), want, f"mode {mode}")


# ---- 7. after edits -----------------------------------------------------------------------------------------------------------------------------

def test_field_of_an_edited_world(world_a):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    try:
        strokes = [{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_SPHERE, "a": (50, 14, 50), "radius": 9, "argb": 0}]
        ctx.brush(strokes)
        solid, colour = _brushed(solid_a, colour_a, strokes)
        blob = np.zeros((10, 12, 14), dtype=bool)  # (X, Z, Y): an L-shaped piece in the air above the crater
        blob[:, :4, :] = True
        blob[:3, :, 5:9] = True
        ctx.write_voxels((46, 30, 44), np.full(blob.shape, 0xFF2299EE, dtype=np.uint32), blob, gpu.BRUSH_FILL)
        solid = solid.copy()
        solid[46:56, 30:44, 44:56] |= blob.transpose(0, 2, 1)
        assert (solid != solid_a).sum() > 1000 and ctx.edit_stats()[0] > 0
        lo, hi = (30, 0, 30), (72, 50, 72)
        for mode in MODES.values():
            want = distancemodel.field(solid, (lo, hi), 8, mode, GROUND)
            assert (want != distancemodel.field(solid_a, (lo, hi), 8, mode, GROUND)).any()
            _same(ctx.distance(lo, hi, 8, mode), want, f"edited, mode {mode}")
    finally:
        ctx.close()


# ---- 8. composition: grow and shrink ------------------------------------------------------------------------------------------------------------

def test_dilate_and_erode_through_torch(world_a):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    solid_a, colour_a, ws_a = world_a
    dev = torch.device("cuda", 0)
    shape = (DIMS[0], DIMS[2], DIMS[1])
    ctx = _context(ws_a)
    try:
        # dilate by 3: the air voxels within 3 of a solid one are filled with one colour
        d = torch.empty(shape, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.distance_device((0, 0, 0), DIMS, 3, d.data_ptr(), TO_SOLID)
        grow = ((d <= 9) & (d > 0)).to(torch.uint8).contiguous()
        paint = torch.full(shape, 0xFF00AA55 - (1 << 32), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ctx.write_voxels_device((0, 0, 0), DIMS, paint.data_ptr(), grow.data_ptr(), gpu.BRUSH_FILL)
        argb, mask = ctx.read_voxels((0, 0, 0), DIMS)
        dilated = distancemodel.field(solid_a, ((0, 0, 0), DIMS), 3, TO_SOLID, GROUND) <= 9  # (X, Z, Y)
        old = solid_a.transpose(0, 2, 1)
        assert dilated.sum() > old.sum() + 10000 and (dilated | old).sum() == dilated.sum()
        assert (mask == dilated).all()
        assert (argb[old] == colour_a.transpose(0, 2, 1)[old]).all() and (argb[dilated & ~old] == 0xFF00AA55).all(), "the old voxels keep their colours"
        # erode by 2: the solid voxels within 2 of an air one are carved
        torch.cuda.synchronize()
        ctx.distance_device((0, 0, 0), DIMS, 2, d.data_ptr(), TO_AIR)
        shrink = ((d <= 4) & (d > 0)).to(torch.uint8).contiguous()
        torch.cuda.synchronize()
        ctx.write_voxels_device((0, 0, 0), DIMS, 0, shrink.data_ptr(), gpu.BRUSH_CARVE)
        _, mask = ctx.read_voxels((0, 0, 0), DIMS, want_argb=False)
        grown = np.ascontiguousarray(dilated.transpose(0, 2, 1))  # (x, y, z)
        eroded = dilated & (distancemodel.field(grown, ((0, 0, 0), DIMS), 2, TO_AIR, GROUND) > 4)
        assert 0 < eroded.sum() < dilated.sum() - 10000 and eroded[2:-2, 2:-2, 0].all() and not eroded[:2].any(), \
            "the ground below keeps the bottom layer, the air beside the world eats into the rim"
        assert (mask == eroded).all()
    finally:
        ctx.close()


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_and_the_next_valid_one(ctx_a):
    L = gpu.lib()
    lo, hi = np.int32([1, 1, 1]), np.int32([5, 5, 5])
    out = np.full(64, -5, dtype=np.int32)

    def call(lo=lo, hi=hi, R=4, mode=TO_SOLID, outside=GROUND, o=out, entry=L.cvx_world_distance):
        return entry(ctx_a._h, None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data, R, mode, outside,
                     None if o is None else o.ctypes.data, None)

    far = np.int32([1, (1 << 30) + 1, 1])
    huge_lo, huge_hi = np.int32([-1024, -1024, -1024]), np.int32([1024, 1024, -512])
    assert (2048 * 2048 * 512) == 1 << 31
    bad = [call(lo=None), call(hi=None), call(o=None), call(o=None, entry=L.cvx_world_distance_device), call(hi=lo), call(lo=hi, hi=lo), call(hi=far), call(lo=-far),
           call(lo=huge_lo, hi=huge_hi), call(R=0), call(R=256), call(R=-1), call(mode=3), call(mode=-1), call(outside=0x40), call(outside=-1)]
    assert bad == [-1] * len(bad), bad
    assert (out == -5).all(), "a rejected call writes nothing"
    with pytest.raises(gpu.CvxError, match="maxDistance"):
        ctx_a.distance(lo, hi, 300)
    with pytest.raises(gpu.CvxError, match="2\\^31"):
        ctx_a.distance(huge_lo, huge_hi, 4)
    assert call() == 0, "the next valid call works"
    _same(out.reshape(4, 4, 4), _sliced(_reference("terrain", 4, TO_SOLID, GROUND, (1, 1, 1), (5, 5, 5)), (1, 1, 1), (1, 1, 1), (5, 5, 5)), "after the errors")
    fresh = gpu.Context(0)
    try:  # before an upload
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.distance((0, 0, 0), (2, 2, 2), 4)
    finally:
        fresh.close()
