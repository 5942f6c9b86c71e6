"""GPU: terrain as height maps out of and into the device-resident world (cvx_world_read_heights[_device], cvx_world_write_heights[_device]).

Reads are compared with the model of tests/heightsmodel.py (an argmax over the numpy volume), element for element.  Writes are applied to a
context and, independently, to the model's volume (the write expanded into dense arrays, tests/densemodel.py), from which the expected world is
built on the host: read back, LOD 0 .. levelCount must equal it byte for byte and the levels above must be the old world's.  The worlds are those
of tests/test_gpu_world_dense.py: the 128 x 64 x 128 terrain and the 32 x 256 x 32 tall world whose runs end at, start at and cross 64 / 128 /
192.  Every case asserts from the model that its input has the property it is named for before it calls the device."""
import numpy as np
import pytest

import densemodel
import heightsmodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _dense, _world
from test_gpu_world_copy import _assert_levels
from test_gpu_world_dense import TALL, _any_world, _tall_solid
from test_gpu_world_edit import DIMS, _colour, _context, _terrain
from test_world_dense_cpu import FILL, CARVE, PAINT, REPLACE, read_boxes
from test_world_heights_cpu import (OPS, WALLED, assert_case_properties, boundaries, column_case_arena, column_case_write, column_cases, write_box)

pytestmark = pytest.mark.gpu


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


# ---- 1. read ------------------------------------------------------------------------------------------------------------------------------------

def _check_read(ctx, solid, colour, lo, hi, name):
    want = heightsmodel.read(solid, colour, (lo, hi))
    got = ctx.read_heights(lo, hi, want_argb=True, want_bottoms=True)
    shape = (hi[0] - lo[0], hi[2] - lo[2])
    assert all(g.shape == shape for g in got) and got[0].dtype == np.int32 and got[1].dtype == np.uint32 and got[2].dtype == np.int32
    for g, w, what in zip(got, want, ("heights", "argb", "bottoms")):
        assert (g == w).all(), f"{name}: {what}"
    return want


def _check_reads(ctx, solid, colour, dims):
    for name, (lo, hi) in read_boxes(dims).items():
        want = _check_read(ctx, solid, colour, lo, hi, name)
        if name == "outside":
            assert (want[0] == lo[1]).all() and not want[1].any() and (want[2] == lo[1]).all(), "none everywhere"
        if name == "sticks out":  # columns outside the world read none; inside, the window is the world's height
            inside = np.zeros(want[0].shape, dtype=bool)
            inside[-lo[0]:dims[0] - lo[0], -lo[2]:dims[2] - lo[2]] = True
            assert (want[0][~inside] == lo[1]).all() and not want[1][~inside].any() and (want[0][inside] > 0).any() and (want[2][inside] >= 0).all()
        if name == "whole":  # any of the three arrays may be left out
            h, a, b = ctx.read_heights(lo, hi)
            assert b is None and (h == want[0]).all() and (a == want[1]).all()
            h, a, b = ctx.read_heights(lo, hi, want_argb=False)
            assert a is None and b is None and (h == want[0]).all()
            only, box_lo, box_hi = np.full(want[2].shape, -9, dtype=np.int32), np.int32(lo), np.int32(hi)
            rc = gpu.lib().cvx_world_read_heights(ctx._h, box_lo.ctypes.data, box_hi.ctypes.data, None, None, only.ctypes.data, None)
            assert rc == 0 and (only == want[2]).all(), "bottoms alone"


def test_read_equals_the_model(ctx_a, world_a):
    solid, colour, _ = world_a
    _check_reads(ctx_a, solid, colour, DIMS)
    # the window's top voxel y1 - 1 in air, inside a run, on a run's top voxel and on its bottom voxel (the slab [34, 38) over column (0, 3)),
    # over footprints of 1 x 1, 5 x 7 and 65 x 3 columns: partial waves, rows shorter and longer than a wave
    column = solid[0, :, 3]
    assert {34, 38} <= boundaries(column) and column[34:38].all() and not column[38:42].any()
    for y1, where in ((41, "in air"), (37, "inside a run"), (38, "on a run's top voxel"), (35, "on a run's bottom voxel")):
        assert column[y1 - 1] == (where != "in air")
        for size in ((1, 1), (5, 7), (65, 3)):
            lo, hi = (0, 20, 3), (size[0], y1, 3 + size[1])
            h, a, b = _check_read(ctx_a, solid, colour, lo, hi, f"y1 - 1 {where}, {size}")
            assert h[0, 0] == (38 if y1 > 38 else y1) and b[0, 0] == 34 and a[0, 0] == colour[0, h[0, 0] - 1, 3]
    assert 65 * 3 % 64 != 0 and 5 * 7 < 64 < 65


def test_read_equals_the_model_in_the_tall_world(ctx_tall, world_tall):
    solid, colour, _ = world_tall
    _check_reads(ctx_tall, solid, colour, TALL)
    for y0, y1 in ((0, 64), (0, 65), (64, 128), (100, 129), (65, 190), (150, 256)):  # windows that end at, above and inside the world's runs
        want = _check_read(ctx_tall, solid, colour, (0, y0, 0), (TALL[0], y1, TALL[2]), f"window [{y0}, {y1})")
        assert (want[0] == y1).any() or y1 == 256, "a run goes through the window's top"
        assert y0 == 0 or (want[0] == y0).any(), "columns with nothing in the window"


# ---- 2. write -----------------------------------------------------------------------------------------------------------------------------------

def _apply(ctx, model, write, level_count):
    """One write on the context and on the model (solid, colour); returns the new model and the milliseconds."""
    at, y1, heights, argb, side, thickness, flags, op = write
    ms = ctx.write_heights(at, y1, heights, argb, side, thickness, flags, op, level_count)
    return heightsmodel.write(model[0], model[1], write_box(write), heights, argb, side, thickness, flags, op), ms


def _hills(shape, at, y0, y1, salt=0):
    """Heights with slopes, plateaus, single-column spikes and pits (cliffs taller than any thickness used here) and values outside the window;
    the top colours and the side colours."""
    x, z = np.meshgrid(np.arange(shape[0]) + at[0], np.arange(shape[1]) + at[2], indexing="ij")
    mid = (y0 + y1) // 2
    heights = (mid + 0.3 * (y1 - y0) * np.sin(x / 5.0 + salt) * np.cos(z / 4.0)).astype(np.int32)
    heights[(x * 7 + z * 3) % 23 == 0] = y1 + 5
    heights[(x * 5 + z * 11) % 29 == 0] = y0 - 2
    heights[(x + 2 * z) % 17 == 0] += 9
    return heights, _colour(x, heights, z, salt=1 + salt), _colour(x, heights, z, salt=2 + salt)


def _write_case(op, thickness, with_side, at=(21, 5, 30), shape=(40, 37), y1=50, flags=0):
    heights, argb, side = _hills(shape, at, at[1], y1, salt=op)
    assert (heights > y1).any() and (heights < at[1]).any() and (np.abs(np.diff(heights, axis=0)) > 7).any() and (np.abs(np.diff(heights, axis=1)) > 7).any()
    return (at, y1, heights, argb, side if with_side else None, thickness, flags, op)


def _check_write(world, write, level_count, label):
    solid_a, colour_a, ws_a = world
    ctx = _context(ws_a)
    try:
        (solid_b, colour_b), ms = _apply(ctx, (solid_a, colour_a), write, level_count)
        assert ms > 0.0
        assert not (solid_b == solid_a).all() or not (colour_b == colour_a).all(), f"{label} changes nothing"
        ws_b = _world(solid_b, colour_b)
        try:
            _assert_levels(ctx, ws_b, ws_a, level_count, label)
        finally:
            ws_b.close()
        return solid_b, colour_b
    finally:
        ctx.close()


@pytest.mark.parametrize("with_side", [True, False], ids=["sideArgb", "no sideArgb"])
@pytest.mark.parametrize("thickness", [0, 1, 2])
@pytest.mark.parametrize("op", sorted(OPS))
def test_write_reads_back_as_the_model(world_a, op, thickness, with_side):
    write = _write_case(OPS[op], thickness, with_side)
    solid_b, colour_b = _check_write(world_a, write, 5, f"{op}, thickness {thickness}, sideArgb {with_side}")
    if OPS[op] in (REPLACE, FILL) and with_side:  # both colours arrive: a top voxel and, below it, a side voxel
        at, y1, heights, argb, side = write[:5]
        k = np.argwhere((heights > at[1] + 2) & (heights <= y1))[0]
        x, z, h = at[0] + k[0], at[2] + k[1], heights[k[0], k[1]]
        assert colour_b[x, h - 1, z] == argb[k[0], k[1]] and (thickness == 1 or colour_b[x, h - 2, z] == side[k[0], k[1]])


@pytest.mark.parametrize("op", sorted(OPS))
def test_write_with_level_count_0_and_a_footprint_aligned_to_nothing(world_a, op):
    write = _write_case(OPS[op], 2, True, at=(3, 2, 5), shape=(13, 70), y1=60)
    assert densemodel.rectangle(write_box(write), DIMS, 0) == (3, 5, 13, 70)
    _check_write(world_a, write, 0, f"{op}, levelCount 0")


def test_walled_rims_go_down_to_the_windows_bottom(world_a):
    write = _write_case(REPLACE, 2, True, at=(40, 20, 50), shape=(9, 11), y1=60, flags=WALLED)
    plain = write[:6] + (0,) + write[7:]
    solid_b, _ = _check_write(world_a, write, 5, "walled")
    solid_p, _ = heightsmodel.write(world_a[0], world_a[1], write_box(plain), *plain[2:])
    rim = np.zeros((9, 11), dtype=bool)
    rim[0, :] = rim[-1, :] = rim[:, 0] = rim[:, -1] = True
    crust_bottom, _ = heightsmodel.spans(write_box(plain), write[2], 2, 0)
    tall = rim & (np.clip(write[2], 20, 60) > 23) & (crust_bottom > 20)
    assert tall.any()
    for bx, bz in np.argwhere(tall):
        h = min(int(write[2][bx, bz]), 60)
        assert solid_b[40 + bx, 20:h, 50 + bz].all() and not solid_p[40 + bx, 20:h, 50 + bz].all(), "a wall under WALLED, a crust without"
    inner = ~rim
    assert (solid_b[41:48, :, 51:60] == solid_p[41:48, :, 51:60]).all() and inner.any(), "the columns inside are the same terrain"


@pytest.mark.parametrize("name,at,shape,y0,y1", [("every side", (-5, 0, -4), (140, 139), -4, 70), ("-x and +y", (-7, 0, 20), (30, 25), 30, 80),
                                                  ("+z and -y", (60, 0, 110), (20, 31), -9, 30)])
def test_footprints_and_windows_that_stick_out(world_a, name, at, shape, y0, y1):
    write = _write_case(REPLACE, 2, True, at=(at[0], y0, at[2]), shape=shape, y1=y1)
    box = write_box(write)
    assert any(box[0][i] < 0 or box[1][i] > DIMS[i] for i in range(3))
    _check_write(world_a, write, 5, f"sticks out: {name}")


@pytest.mark.parametrize("at,y1", [((DIMS[0] + 1, 0, 0), 20), ((2, DIMS[1], 2), DIMS[1] + 9), ((2, -9, 2), 0)], ids=["beside", "above", "below"])
def test_a_box_wholly_outside_writes_nothing_and_reads_none(world_a, at, y1):
    _, _, ws_a = world_a
    ctx = _context(ws_a)
    try:
        heights = np.full((4, 5), y1, dtype=np.int32)
        assert ctx.write_heights(at, y1, heights, np.full((4, 5), 0xFF00FF00, dtype=np.uint32), None, 0) == 0.0
        _assert_levels(ctx, ws_a, ws_a, 5, "wholly outside")
        assert ctx.edit_stats()[1:] == (0, 0)
        h, a, b = ctx.read_heights(at, (at[0] + 4, y1, at[2] + 5), want_bottoms=True)
        assert (h == at[1]).all() and not a.any() and (b == at[1]).all()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(column_cases(TALL[1])))
def test_column_cases_in_the_tall_world(world_tall, name):
    """The column cases of the CPU test in column (5, 6) of the tall world: a dense REPLACE over the whole column gives it the case's arena
    spans, the second write is the case."""
    solid_a, colour_a, ws_a = world_tall
    dim_y = TALL[1]
    case = column_cases(dim_y)[name]
    case_solid, case_colour = column_case_arena(dim_y, case)
    write = column_case_write(case, column=(5, 6))
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws_a)
        ctx.write_voxels((5, 0, 6), np.ascontiguousarray(case_colour.transpose(0, 2, 1)), np.ascontiguousarray(case_solid.transpose(0, 2, 1)), REPLACE, 5)
        model = densemodel.write(solid_a, colour_a, ((5, 0, 6), (6, dim_y, 7)), case_colour.transpose(0, 2, 1), case_solid.transpose(0, 2, 1), REPLACE)
        assert (model[0][5, :, 6] == case_solid[0, :, 0]).all()
        model, ms = _apply(ctx, model, write, 5)
        assert ms > 0.0
        # the column has the property the case is named for (the checks of the CPU test, for this case alone)
        others = {n: (heightsmodel.write(*column_case_arena(dim_y, c), write_box(column_case_write(c)), *column_case_write(c)[2:])) for n, c in column_cases(dim_y).items()}
        after = {n: (s[0, :, 0], c[0, :, 0]) for n, (s, c) in others.items()}
        assert_case_properties(dim_y, after)
        assert (model[0][5, :, 6] == after[name][0]).all() and (model[1][5, :, 6] == after[name][1]).all(), "the case's column, in the tall world"
        ws_b = _any_world(TALL, *model)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, name)
        finally:
            ws_b.close()
    finally:
        ctx.close()


def test_windows_at_the_tall_worlds_run_ends(world_tall):
    """Windows and heights at the heights the tall world's runs end at, start at and cross (64, 128, 192): written terrain that merges with the
    arena's [40, 64) from above and with [128, 150) from below, a window cut out of [60, 190), a repaint of [40, 64)'s top."""
    solid_a, colour_a, ws_a = world_tall
    shape = (TALL[0], TALL[2])
    x, z = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    top, side = _colour(x, x * 0 + 7, z, salt=3), _colour(x, x * 0 + 9, z, salt=4)
    flat = lambda h: np.full(shape, h, dtype=np.int32)  # noqa: E731
    writes = [((0, 64, 0), 128, flat(128), top, side, 0, 0, FILL), ((0, 100, 0), 192, flat(128), top, side, 0, 0, REPLACE),
              ((0, 40, 0), 64, flat(64), top, None, 3, 0, PAINT), ((0, 60, 0), 190, flat(150), None, None, 0, 0, CARVE)]
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws_a)
        model = (solid_a, colour_a)
        for k, write in enumerate(writes):
            before = model
            model, ms = _apply(ctx, model, write, 5)
            assert ms > 0.0 and (not (model[0] == before[0]).all() or not (model[1] == before[1]).all()), f"write {k} changes something"
            if k == 0:
                columns = [(cx, cz) for cx in range(TALL[0]) for cz in range(TALL[2])]
                assert any(solid_a[cx, 40:64, cz].all() and not solid_a[cx, 64, cz] and model[0][cx, 40:128, cz].all() for cx, cz in columns), "merges across 64"
                assert any(solid_a[cx, 128:150, cz].all() and not solid_a[cx, 127, cz] and model[0][cx, 64:150, cz].all() for cx, cz in columns), "merges across 128"
            ws_b = _any_world(TALL, *model)
            try:
                _assert_levels(ctx, ws_b, ws_a, 5, f"write {k}")
            finally:
                ws_b.close()
    finally:
        ctx.close()


# ---- 3. equivalence with the dense write --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op,thickness,flags", [(REPLACE, 2, 0), (FILL, 0, 0), (PAINT, 7, WALLED), (CARVE, 1, 0)])
def test_the_write_is_the_dense_write_of_its_expansion(world_a, op, thickness, flags):
    _, _, ws_a = world_a
    write = _write_case(op, thickness, True, at=(-3, 4, 17), shape=(50, 41), y1=58, flags=flags)
    at, y1, heights, argb, side = write[:5]
    argb3, mask3 = heightsmodel.expand(write_box(write), heights, argb, side, thickness, flags)
    assert mask3.any() and not mask3.all() and mask3.shape == (50, 41, 54)
    one, two = _context(ws_a), _context(ws_a)
    try:
        assert one.write_heights(at, y1, heights, argb, side, thickness, flags, op, 5) > 0.0
        assert two.write_voxels(at, argb3, mask3, op, 5) > 0.0
        changed = False
        for level in range(6):
            a, b = one.read_level(level), two.read_level(level)
            assert a == b, f"LOD {level}"
            changed = changed or a[0] != ws_a.storage(level).tobytes()
        assert changed
    finally:
        one.close()
        two.close()


# ---- 4. round trip ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("thickness", [1, 2, 7])
def test_reading_what_was_written_returns_it(world_a, thickness):
    _, _, ws_a = world_a
    ctx = _context(ws_a)
    try:
        at, shape, y1 = (10, 3, 12), (66, 45), 61
        heights, argb, side = _hills(shape, at, at[1], y1)
        ctx.write_heights(at, y1, np.full(shape, at[1], dtype=np.int32), argb, None, 0, 0, REPLACE, 5)  # H == y0 everywhere: the window is emptied
        h, a, b = ctx.read_heights(at, (at[0] + shape[0], y1, at[2] + shape[1]), want_bottoms=True)
        assert (h == at[1]).all() and not a.any() and (b == at[1]).all()
        ctx.write_heights(at, y1, heights, argb, side, thickness, 0, REPLACE, 5)
        want_b, want_h = heightsmodel.spans(write_box((at, y1, heights)), heights, thickness, 0)
        assert (want_h > want_b).any() and (want_h == want_b).any() and (want_h - want_b > thickness).any(), "crusts, columns left empty, closed cliffs"
        h, a, b = ctx.read_heights(at, (at[0] + shape[0], y1, at[2] + shape[1]), want_bottoms=True)
        assert (h == want_h).all() and (b == want_b).all() and (a == np.where(want_h > want_b, argb, 0)).all()
    finally:
        ctx.close()


# ---- 5. torch tensors ---------------------------------------------------------------------------------------------------------------------------

def test_a_terrain_tool_that_never_leaves_the_device(world_a):
    """read_heights_device into tensors, a torch blur of the heights, write_heights_device: everything on the context's stream."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    solid_a, colour_a, ws_a = world_a
    dev = torch.device("cuda", 0)
    ctx = _context(ws_a)
    try:
        lo, hi = (9, 0, 14), (109, 64, 91)
        shape = (hi[0] - lo[0], hi[2] - lo[2])
        stream = torch.cuda.Stream(device=dev)
        ctx.set_stream(stream.cuda_stream)
        with torch.cuda.stream(stream):
            heights = torch.full(shape, -77, dtype=torch.int32, device=dev)
            argb = torch.full(shape, -1, dtype=torch.int32, device=dev)
            ctx.read_heights_device(lo, hi, heights.data_ptr(), argb.data_ptr(), 0)
            smooth = torch.nn.functional.avg_pool2d(heights.to(torch.float32)[None, None], 5, stride=1, padding=2, count_include_pad=False)[0, 0]
            smooth = torch.round(smooth).to(torch.int32).contiguous()
            ms = ctx.write_heights_device(lo, hi, smooth.data_ptr(), argb.data_ptr(), 0, 2, 0, REPLACE, 5)
        stream.synchronize()
        assert ms > 0.0
        want_h, want_a, _ = heightsmodel.read(solid_a, colour_a, (lo, hi))
        host_h, host_a, host_s = heights.cpu().numpy(), argb.cpu().numpy().view(np.uint32), smooth.cpu().numpy()
        assert (host_h == want_h).all() and (host_a == want_a).all(), "the tensors hold the read"
        assert (host_s != host_h).any() and host_s.min() > 0, "the blur moved the ground"
        model = heightsmodel.write(solid_a, colour_a, (lo, hi), host_s, host_a, None, 2, 0, REPLACE)
        ws_b = _world(*model)
        try:
            _assert_levels(ctx, ws_b, ws_a, 5, "the smoothed terrain")
        finally:
            ws_b.close()
        ctx.set_stream(None)
    finally:
        ctx.close()


# ---- 6. errors ----------------------------------------------------------------------------------------------------------------------------------

def test_a_terrain_over_the_format_limits_is_rejected_whole():
    """thickness 0 over a window of 32768 voxels makes one run of 32768 (RLEColumn keeps lengths in shorts), in the 32 x 32768 x 32 world of
    tests/test_gpu_world_edit_rejections.py: CVX_ERR_CAPACITY from the pipeline's check behind the count kernel, and the level stays as it was."""
    dims = (32, 32768, 32)
    xs, zs = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    xs, zs = xs.ravel(), zs.ravel()
    ys = (xs * 7 + zs * 3) % 50
    ws = host.WorldSet.from_voxels(dims, xs.astype(np.int32), ys.astype(np.int32), zs.astype(np.int32), _colour(xs, ys, zs), threads=4)
    heights = np.full((3, 2), 100, dtype=np.int32)
    heights[1, 1] = dims[1]
    assert dims[1] - 0 > 32767 and heights.max() == dims[1]  # one column solid over the whole window: a run longer than a short holds
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        before = ctx.read_level(0)[0]
        assert before == ws.storage(0).tobytes()
        stats = ctx.edit_stats()
        with pytest.raises(gpu.CvxError, match=r"error -4: a written column would need .* a run longer than 32767 voxels"):
            ctx.write_heights((3, 0, 3), dims[1], heights, np.full((3, 2), 0xFF000000, dtype=np.uint32), None, 0, 0, REPLACE, 5)
        assert ctx.read_level(0)[0] == before
        assert ctx.edit_stats() == stats
        assert ctx.write_heights((3, 0, 3), dims[1], np.minimum(heights, 32767), np.full((3, 2), 0xFF000000, dtype=np.uint32), None, 0, 0, REPLACE, 5) > 0.0
        assert ctx.read_level(0)[0] != before, "32767 fits"
    finally:
        ctx.close()
        ws.close()


def test_rejected_calls_leave_the_world_alone(world_a):
    _, _, ws_a = world_a
    ctx = _context(ws_a)
    L = gpu.lib()
    try:
        before = ctx.read_level(0)
        h = np.full((4, 4), 20, dtype=np.int32)
        argb = np.full((4, 4), 0xFF445566, dtype=np.uint32)
        out = np.zeros((4, 4), dtype=np.int32)
        lo, hi = np.int32([1, 1, 1]), np.int32([5, 30, 5])
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731

        def read(lo, hi, heights=out, colours=argb, bottoms=out, device=False):
            call = L.cvx_world_read_heights_device if device else L.cvx_world_read_heights
            return call(ctx._h, ptr(lo), ptr(hi), ptr(heights), ptr(colours), ptr(bottoms), None), L.cvx_last_error(ctx._h).decode()

        def write(lo, hi, heights=h, colours=argb, side=None, thickness=1, flags=0, op=REPLACE, levels=5, device=False):
            call = L.cvx_world_write_heights_device if device else L.cvx_world_write_heights
            return call(ctx._h, ptr(lo), ptr(hi), ptr(heights), ptr(colours), ptr(side), thickness, flags, op, levels, None), L.cvx_last_error(ctx._h).decode()

        far = np.int32([9, (1 << 30) + 1, 9])
        wide_lo, wide_hi = np.int32([0, 0, 0]), np.int32([1 << 16, 1, 1 << 15])
        assert (1 << 16) * (1 << 15) == 1 << 31
        bad = {
            "read: NULL boxMin": (read(None, hi), "NULL box"), "read: NULL boxMax": (read(lo, None), "NULL box"),
            "read: an empty axis": (read(lo, np.int32([5, 30, 1])), "is empty"), "read: an empty window": (read(lo, np.int32([5, 1, 5])), "is empty"),
            "read: beyond 2^30": (read(lo, far), "beyond 2^30"), "read: beyond -2^30": (read(-far, hi), "beyond 2^30"),
            "read: 2^31 columns": (read(wide_lo, wide_hi), "2^31 or more columns"),
            "read: all outputs NULL": (read(lo, hi, None, None, None), "all NULL"),
            "read_device: all outputs NULL": (read(lo, hi, None, None, None, device=True), "all NULL"),
            "write: NULL boxMin": (write(None, hi), "NULL box"), "write: NULL boxMax": (write(lo, None), "NULL box"),
            "write: an empty axis": (write(hi, lo), "is empty"), "write: beyond 2^30": (write(lo, far), "beyond 2^30"),
            "write: 2^31 columns": (write(wide_lo, wide_hi), "2^31 or more columns"),
            "write: heights NULL": (write(lo, hi, None), "heights is NULL"), "write_device: heights NULL": (write(lo, hi, None, device=True), "heights is NULL"),
            "write: argb NULL, REPLACE": (write(lo, hi, h, None), "argb is NULL"), "write: argb NULL, FILL": (write(lo, hi, h, None, op=FILL), "argb is NULL"),
            "write: argb NULL, PAINT": (write(lo, hi, h, None, op=PAINT), "argb is NULL"),
            "write: thickness -1": (write(lo, hi, thickness=-1), "thickness -1 outside 0 .. 32767"),
            "write: thickness 32768": (write(lo, hi, thickness=32768), "thickness 32768 outside 0 .. 32767"),
            "write: unknown flag bits": (write(lo, hi, flags=WALLED | 2), "unknown flag bits 0x2"), "write: flags -1": (write(lo, hi, flags=-1), "unknown flag bits"),
            "write: op 4": (write(lo, hi, op=4), "bad op 4"), "write: op -1": (write(lo, hi, op=-1), "bad op -1"),
            "write: levelCount 6": (write(lo, hi, levels=6), "levelCount 6 outside"), "write: levelCount -1": (write(lo, hi, levels=-1), "levelCount -1 outside"),
        }
        for name, ((code, message), part) in bad.items():
            assert code == -1 and part in message, f"{name}: {code} {message!r}"
        assert ctx.read_level(0) == before and ctx.edit_stats()[1:] == (0, 0)
        with pytest.raises(gpu.CvxError, match="thickness"):
            ctx.write_heights((1, 1, 1), 30, h, argb, thickness=40000)
        code, _ = write(lo, hi, h, None, op=CARVE, thickness=0)
        assert code == 0, "a CARVE takes heights alone"
        assert ctx.read_level(0) != before
    finally:
        ctx.close()
    fresh = gpu.Context(0)
    try:  # before an upload
        with pytest.raises(gpu.CvxError, match="error -3: .*not been uploaded"):
            fresh.read_heights((0, 0, 0), (2, 2, 2))
        with pytest.raises(gpu.CvxError, match="error -3: .*not been uploaded"):
            fresh.write_heights((0, 0, 0), 2, np.ones((2, 2), dtype=np.int32), np.ones((2, 2), dtype=np.uint32))
    finally:
        fresh.close()
