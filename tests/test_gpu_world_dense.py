"""GPU: dense voxel boxes out of and into the device-resident world (cvx_world_read_voxels[_device], cvx_world_write_voxels[_device]).

Reads are compared with the dense numpy model of tests/densemodel.py, element for element.  Writes are applied to a context and, independently,
to the model's volume, from which the expected world is built on the host (host.WorldSet.from_voxels): read back, LOD 0 .. levelCount must equal
it byte for byte and the levels above must be the old world's.  The worlds: the 128 x 64 x 128 terrain of tests/test_gpu_world_edit.py (one
64-voxel step of the write kernels per column) and a 32 x 256 x 32 world (four steps; the builder takes powers of two only, 256 is the nearest
height above two waves) for the runs that end at, start at and cross the steps.  Every case asserts from the model that its input has the
property it is named for before it calls the device.

The over-limit rejections (a run above 32767 voxels, a colour index above 32767, more than 65535 runs) are covered on the CPU
(tests/test_world_dense_cpu.py) through the same step functions the kernels run; on the device the run above 32767 voxels is rejected in
tests/test_gpu_world_edit_rejections.py, on the 32 x 32768 x 32 world of the brush's and the copy's over-limit tests (tests/limitworlds.py
offers no world tall enough)."""
import numpy as np
import pytest

import densemodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _check_picks, _dense, _world
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _colour, _context, _frames, _terrain
from test_world_dense_cpu import FILL, CARVE, PAINT, REPLACE, _box, column_case_world, column_cases, random_dense, read_boxes, world_cases

pytestmark = pytest.mark.gpu

TALL = (32, 256, 32)
STEPS = (64, 128, 192)  # the write kernels walk a column of 256 voxels in four steps: the voxels below and above these are in different steps


def _tall_solid():
    """Terrain with runs that end exactly below a step ([40, 64)), start exactly at one ([64, 100), [128, 150)), end at 127 | 128 and cross
    three steps ([60, 190))."""
    dx, dy, dz = TALL
    x, y, z = np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij")
    solid = y < 12 + (x * 3 + z * 5) % 9
    kind = (x // 2 + z // 3) % 5
    solid |= (kind == 0) & (y >= 40) & (y < 64)
    solid |= (kind == 1) & (y >= 64) & (y < 100)
    solid |= (kind == 2) & (y >= 100) & (y < 128)
    solid |= (kind == 3) & (y >= 60) & (y < 190)
    solid |= (kind == 4) & (y >= 128) & (y < 150)
    return solid


def _any_world(dims, solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


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


def _boundaries(column):
    """The heights y at which a column (bool over y) changes between y - 1 and y."""
    return set((np.nonzero(column[1:] != column[:-1])[0] + 1).tolist())


# ---- 1. read ------------------------------------------------------------------------------------------------------------------------------------

def _check_reads(ctx, solid, colour, dims):
    mixed = 0
    for name, (lo, hi) in read_boxes(dims).items():
        want_argb, want_mask = densemodel.read(solid, colour, (lo, hi))
        inside = densemodel.rectangle((lo, hi), dims, 0) is not None
        assert name != "outside" or not inside
        mixed += bool(want_mask.any() and not want_mask.all())
        argb, mask = ctx.read_voxels(lo, hi)
        assert argb.shape == want_argb.shape == (hi[0] - lo[0], hi[2] - lo[2], hi[1] - lo[1]) and mask.dtype == np.bool_
        assert (argb == want_argb).all() and (mask == want_mask).all(), f"{name}: both arrays"
        only_argb, none = ctx.read_voxels(lo, hi, want_solid=False)
        assert none is None and (only_argb == want_argb).all(), f"{name}: argb only"
        none, only_mask = ctx.read_voxels(lo, hi, want_argb=False)
        assert none is None and (only_mask == want_mask).all(), f"{name}: solid only"
        if name == "sticks out":  # entries outside the world are 0
            outside = np.ones(want_mask.shape, dtype=bool)
            outside[-lo[0]:dims[0] - lo[0], -lo[2]:dims[2] - lo[2], -lo[1]:dims[1] - lo[1]] = False
            assert outside.sum() == outside.size - dims[0] * dims[1] * dims[2] and not argb[outside].any() and not mask[outside].any()
    assert mixed >= 6, "most boxes hold solid and air"


def test_read_equals_the_volume(ctx_a, world_a):
    solid, colour, _ = world_a
    boxes = read_boxes(DIMS)
    assert {b[1][1] - b[0][1] for b in boxes.values()} >= {1, 3, 63, 64, 65, 129} and all(b[0][1] % 64 for n, b in boxes.items() if n.startswith("height"))
    assert (boxes["5 x 7 columns of 3"][1][0] - boxes["5 x 7 columns of 3"][0][0]) * (boxes["5 x 7 columns of 3"][1][2] - boxes["5 x 7 columns of 3"][0][2]) % (64 // 3) != 0
    _check_reads(ctx_a, solid, colour, DIMS)


def test_read_equals_the_volume_in_the_tall_world(ctx_tall, world_tall):
    solid, colour, _ = world_tall
    columns = solid.transpose(0, 2, 1).reshape(-1, TALL[1])
    assert all(any(s in _boundaries(c) for c in columns) for s in (64, 128)), "runs that end and start at the steps"
    _check_reads(ctx_tall, solid, colour, TALL)


# ---- 2. write -----------------------------------------------------------------------------------------------------------------------------------

def _apply(ctx, model, write, level_count):
    """One write on the context and on the model (solid, colour); returns the new model and the milliseconds."""
    at, argb, mask, op = write
    ms = ctx.write_voxels(at, argb, mask, op, level_count)
    return densemodel.write(model[0], model[1], _box(at, argb if argb is not None else mask), argb, mask, op), ms


CASES = world_cases(DIMS, np.random.default_rng(11))


@pytest.mark.parametrize("name,level_count", [(n, 5) for n in sorted(CASES)] + [(f"{op}, {m}", 0) for op in ("fill", "carve", "paint", "replace")
                                                                                    for m in ("mask", "no mask")])
def test_write_reads_back_as_the_model(world_a, name, level_count):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    try:
        (solid_b, colour_b), ms = _apply(ctx, (solid_a, colour_a), CASES[name], level_count)
        if name.startswith("wholly"):
            assert ms == 0.0
            _assert_levels(ctx, ws_a, ws_a, 5, name)
            assert ctx.edit_stats()[1:] == (0, 0)
            return
        assert ms > 0.0
        assert not (solid_b == solid_a).all() or not (colour_b == colour_a).all(), f"{name} changes nothing"
        ws_b = _world(solid_b, colour_b)
        try:
            _assert_levels(ctx, ws_b, ws_a, level_count, f"{name}, levelCount {level_count}")
        finally:
            ws_b.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(column_cases(TALL[1])))
def test_column_cases_in_the_tall_world(world_tall, name):
    """The column cases of the CPU test in column (5, 6) of the tall world: a first REPLACE over the whole column gives it the case's arena
    spans, the second write is the case."""
    solid_a, colour_a, ws_a = world_tall
    dim_y = TALL[1]
    case_solid, case_colour, (at, argb, mask, op) = column_case_world(dim_y, column_cases(dim_y)[name])
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws_a)
        first = ((5, 0, 6), np.ascontiguousarray(case_colour.transpose(0, 2, 1)), np.ascontiguousarray(case_solid.transpose(0, 2, 1)), REPLACE)
        model, _ = _apply(ctx, (solid_a, colour_a), first, 5)
        assert (model[0][5, :, 6] == case_solid[0, :, 0]).all()
        before = model[0][5, :, 6].copy()
        model, ms = _apply(ctx, model, ((5, at[1], 6), argb, mask, op), 5)
        column = model[0][5, :, 6]
        assert ms > 0.0
        if name == "emptied":
            assert not column.any()
        elif name.startswith("merged"):
            assert _boundaries(column) == {1, dim_y - 1} and len(_boundaries(before)) == 4, "one run where there were two"
        elif name.startswith("alternating"):
            assert len(_boundaries(column)) == dim_y - 1
        else:
            assert (column == before).all() and (model[1][5, :, 6] != case_colour[0, :, 0])[before].all(), "paint recolours the solid voxels only"
        ws_b = _any_world(TALL, *model)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, name)
        finally:
            ws_b.close()
    finally:
        ctx.close()


def test_runs_at_and_across_the_steps(world_tall):
    """Written runs that end exactly at 63 | 64 and 127 | 128, one that spans three steps, and fills that merge with the arena's runs across a
    step, in neighbouring columns of one box."""
    solid_a, colour_a, ws_a = world_tall
    spans = [[(10, 64)], [(64, 128)], [(60, 190)], [(0, 64), (65, 128), (129, 192), (193, 256)], [(63, 65), (127, 129), (191, 193)]]
    shape = (len(spans), 3, TALL[1])
    mask = np.zeros(shape, dtype=bool)
    for k, column in enumerate(spans):
        for lo, hi in column:
            mask[k, :, lo:hi] = True
    argb = _colour(*np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij"), salt=5).astype(np.uint32)
    assert _boundaries(mask[0, 0]) == {10, 64} and _boundaries(mask[1, 0]) == {64, 128} and _boundaries(mask[2, 0]) == {60, 190}
    assert {s // 64 for s in range(60, 190)} == {0, 1, 2}, "three steps"
    for op in (REPLACE, FILL):
        ctx = gpu.Context(0)
        try:
            ctx.upload_world(ws_a)
            model, ms = _apply(ctx, (solid_a, colour_a), ((4, 0, 9), argb, mask, op), 5)
            assert ms > 0.0
            if op == FILL:  # the arena's [40, 64) and the written [64, 128) become one run across the step
                merged = [(x, z) for x in range(4, 9) for z in range(9, 12) if solid_a[x, 40:64, z].all() and not solid_a[x, 64, z] and model[0][x, 40:128, z].all()]
                assert merged, "no column merges a run of the arena with a written one across y = 64"
            ws_b = _any_world(TALL, *model)
            try:
                _assert_levels(ctx, ws_b, ws_a, 5, f"op {op}")
            finally:
                ws_b.close()
        finally:
            ctx.close()


# ---- 3. round trips -----------------------------------------------------------------------------------------------------------------------------

def test_writing_what_was_read_changes_nothing(world_a):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    try:
        argb, mask = ctx.read_voxels((0, 0, 0), DIMS)
        assert mask.any() and not mask.all()
        assert ctx.write_voxels((0, 0, 0), argb, mask, REPLACE, 5) > 0.0
        _assert_levels(ctx, ws_a, ws_a, 5, "write(REPLACE, read(world))")
        # ... and a box that sticks out, without the mask: the zeros are air
        lo, hi = (-3, -2, 100), (40, 70, 131)
        argb, _ = ctx.read_voxels(lo, hi, want_solid=False)
        assert ctx.write_voxels(lo, argb, None, REPLACE, 5) > 0.0
        _assert_levels(ctx, ws_a, ws_a, 5, "write(REPLACE, read(box))")
    finally:
        ctx.close()


def test_reading_what_was_written_returns_it(world_a):
    _, _, ws_a = world_a
    rng = np.random.default_rng(3)
    ctx = _context(ws_a)
    try:
        at, shape = (100, 40, -5), (40, 30, 50)  # (X, Z, Y): sticks out in +x, +y and -z
        argb, mask = random_dense(rng, shape, with_mask=True)
        assert (mask & (argb == 0)).any()
        ctx.write_voxels(at, argb, mask, REPLACE, 5)
        lo, hi = _box(at, argb)
        got_argb, got_mask = ctx.read_voxels(lo, hi)
        inside = np.zeros(shape, dtype=bool)
        inside[:DIMS[0] - at[0], -at[2]:, :DIMS[1] - at[1]] = True
        assert inside.any() and not inside.all()
        assert (got_mask == (mask & inside)).all() and (got_argb == np.where(mask & inside, argb, 0)).all()
    finally:
        ctx.close()


# ---- 4. the scan's chunk edges ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size_x,size_z", [(63, 65), (64, 64), (64, 65)])
def test_footprints_around_the_scan_chunk(world_a, size_x, size_z):
    """4095, 4096 and 4160 columns with levelCount 0: below, at and above one chunk of the offset scan."""
    solid_a, colour_a, ws_a = world_a
    assert (size_x * size_z in (4095, 4096, 4160)) and 4095 < 4096 < 4160
    argb, mask = random_dense(np.random.default_rng(size_x * size_z), (size_x, size_z, 23), with_mask=True)
    ctx = _context(ws_a)
    try:
        model, ms = _apply(ctx, (solid_a, colour_a), ((31, 9, 17), argb, mask, REPLACE), 0)
        assert ms > 0.0 and densemodel.rectangle(_box((31, 9, 17), argb), DIMS, 0) == (31, 17, size_x, size_z)
        ws_b = _world(*model)
        try:
            _assert_levels(ctx, ws_b, ws_a, 0, f"{size_x} x {size_z} columns")
        finally:
            ws_b.close()
    finally:
        ctx.close()


# ---- 5. rendering and picks ---------------------------------------------------------------------------------------------------------------------

def test_a_sequence_of_writes_renders_and_picks_as_the_rebuild(world_a):
    solid_a, colour_a, ws_a = world_a
    rng = np.random.default_rng(21)
    x, z, y = np.meshgrid(np.arange(40), np.arange(36), np.arange(44), indexing="ij")
    block = np.where((x - 20) ** 2 + (z - 18) ** 2 + (y - 22) ** 2 < 18 ** 2, _colour(x, y, z, salt=3), 0).astype(np.uint32)  # a generated ball
    prefab, _ = random_dense(rng, (30, 30, 20), zeros=0.5, with_mask=False)
    hole = rng.random((25, 40, 30)) < 0.7
    paint = np.full((50, 50, 64), 0xFF3366CC, dtype=np.uint32)
    writes = [((30, 10, 40), block, None, REPLACE), ((110, 50, -10), prefab, None, FILL), ((60, 0, 60), None, hole, CARVE), ((20, 0, 70), paint, None, PAINT)]
    assert 110 + 30 > DIMS[0] and 50 + 20 > DIMS[1], "the prefab lies partly outside the world"
    ctx = _context(ws_a)
    try:
        model = (solid_a, colour_a)
        for w in writes:
            before = model
            model, ms = _apply(ctx, model, w, 5)
            assert ms > 0.0 and (not (model[0] == before[0]).all() or not (model[1] == before[1]).all()), "every write changes something"
        ws_b = _world(*model)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, "the sequence")
            visited = _check_world(ctx, ws_b, _frames(ws_a)[1:3], "the sequence")
            assert visited.sum() > 0
            _check_picks(ctx, model[0], model[1], np.random.default_rng(7), 4096, "the sequence")
        finally:
            ws_b.close()
    finally:
        ctx.close()


# ---- 6. torch tensors ---------------------------------------------------------------------------------------------------------------------------

def test_torch_tensors_go_in_and_come_out(world_a):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    solid_a, colour_a, ws_a = world_a
    dev = torch.device("cuda", 0)
    ctx = _context(ws_a)
    try:
        # generated on the device: a sine surface with a colour per height, (X, Z, Y)
        lo, hi = (16, 4, 24), (80, 60, 72)
        xs, zs, ys = torch.meshgrid(torch.arange(64, device=dev), torch.arange(48, device=dev), torch.arange(56, device=dev), indexing="ij")
        height = (28 + 12 * torch.sin(xs / 6.0) * torch.cos(zs / 5.0)).to(torch.int64)
        argb = torch.where(ys < height, 0xFF000000 + ys * 0x010203 + xs, torch.zeros_like(ys)).to(torch.int64)
        argb_i32 = torch.where(argb >= 2 ** 31, argb - 2 ** 32, argb).to(torch.int32).contiguous()  # the colour words in 32 bits
        torch.cuda.synchronize()
        ms = ctx.write_voxels_device(lo, hi, argb_i32.data_ptr(), 0, REPLACE, 5)
        assert ms > 0.0
        host_argb = (argb.cpu().numpy() & 0xFFFFFFFF).astype(np.uint32)
        assert (host_argb != 0).any() and (host_argb == 0).any()
        model = densemodel.write(solid_a, colour_a, (lo, hi), host_argb, None, REPLACE)
        ws_b = _world(*model)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, "a tensor written")
        finally:
            ws_b.close()
        # read back into tensors on a stream of torch's (the write has finished: the call returns when the edit is done)
        out_argb = torch.full((64, 48, 56), -1, dtype=torch.int32, device=dev)
        out_mask = torch.full((64, 48, 56), 7, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            ctx.read_voxels_device(lo, hi, out_argb.data_ptr(), out_mask.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        want = torch.from_numpy(host_argb.view(np.int32)).to(dev)
        assert torch.equal(out_argb, want) and torch.equal(out_mask, (want != 0).to(torch.uint8))
        # a mask alone carves
        carve = (xs + zs + ys) % 3 == 0
        carve_u8 = carve.to(torch.uint8).contiguous()
        torch.cuda.synchronize()
        assert ctx.write_voxels_device(lo, hi, 0, carve_u8.data_ptr(), CARVE, 5) > 0.0
        model = densemodel.write(model[0], model[1], (lo, hi), None, carve.cpu().numpy(), CARVE)
        got_argb, got_mask = ctx.read_voxels((0, 0, 0), DIMS)
        want_argb, want_mask = densemodel.read(model[0], model[1], ((0, 0, 0), DIMS))
        assert (got_argb == want_argb).all() and (got_mask == want_mask).all()
    finally:
        ctx.close()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_leave_the_world_alone(world_a):
    _, _, ws_a = world_a
    ctx = _context(ws_a)
    L = gpu.lib()
    try:
        before = ctx.read_level(0)
        argb = np.full((4, 4, 4), 0xFF445566, dtype=np.uint32)
        mask = np.ones((4, 4, 4), dtype=bool)
        lo, hi = np.int32([1, 1, 1]), np.int32([5, 5, 5])
        u8 = mask.view(np.uint8)

        def read(lo, hi, a=argb, s=u8):
            return L.cvx_world_read_voxels(ctx._h, None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
                                           None if a is None else a.ctypes.data, None if s is None else s.ctypes.data, None)

        def write(lo, hi, a=argb, s=u8, op=REPLACE, levels=5):
            return L.cvx_world_write_voxels(ctx._h, None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
                                            None if a is None else a.ctypes.data, None if s is None else s.ctypes.data, op, levels, None)

        far = np.int32([1, (1 << 30) + 1, 1])
        huge_lo, huge_hi = np.int32([-1024, -1024, -1024]), np.int32([1024, 1024, -512])
        assert (2048 * 2048 * 512) == 1 << 31
        bad = [read(None, hi), read(lo, None), read(lo, lo), read(lo, far), read(-far, hi), read(huge_lo, huge_hi), read(lo, hi, None, None),
               write(None, hi), write(lo, None), write(hi, lo), write(lo, far), write(huge_lo, huge_hi), write(lo, hi, op=4), write(lo, hi, op=-1),
               write(lo, hi, levels=6), write(lo, hi, levels=-1), write(lo, hi, None, u8, FILL), write(lo, hi, None, u8, REPLACE), write(lo, hi, None, u8, PAINT),
               write(lo, hi, None, None, CARVE),
               L.cvx_world_read_voxels_device(ctx._h, lo.ctypes.data, hi.ctypes.data, None, None, None),
               L.cvx_world_write_voxels_device(ctx._h, lo.ctypes.data, hi.ctypes.data, None, None, REPLACE, 5, None)]
        assert bad == [-1] * len(bad), bad
        assert ctx.read_level(0) == before and ctx.edit_stats()[1:] == (0, 0)
        with pytest.raises(gpu.CvxError, match="2\\^31"):
            ctx.read_voxels(huge_lo, huge_hi)
        with pytest.raises(gpu.CvxError, match="bad op"):
            ctx.write_voxels((1, 1, 1), argb, mask, 9)
        assert write(lo, hi, None, u8, CARVE) == 0, "a CARVE takes a mask alone"
        assert ctx.read_level(0) != before
    finally:
        ctx.close()
    fresh = gpu.Context(0)
    try:  # before an upload
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.read_voxels((0, 0, 0), (2, 2, 2))
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.write_voxels((0, 0, 0), np.ones((2, 2, 2), dtype=np.uint32))
    finally:
        fresh.close()
