"""GPU: the rejections of the column-edit pipeline (cvxi::RoundEditRectangle / cvxi::ColumnEdit, cvx_edit.hip), through every call that runs it.

Two paths every caller shares: a rectangle that cannot be rounded out to 2^levelCount because the world is narrower than that (rejected before the
pipeline allocates anything) and a column the blob's format cannot hold (rejected after the count kernel, the scan and the copy back).  Either way
the level must read back byte for byte as it was uploaded and cvx_world_edit_stats must not move.  Each call is given real work: the test
asserts from the numpy volume, with the project's dense models, that the world holds what the call would change."""
import numpy as np
import pytest

import cavitymodel
import piecesmodel
from cpuvox_amd import gpu, host
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import _colour
from test_world_copy_cpu import _placement

pytestmark = pytest.mark.gpu

NARROW = (16, 64, 16)  # 16 columns a side: narrower than 2^5
BLOCK = (slice(4, 6), slice(20, 22), slice(4, 6))  # the floating block
CAVITY = (10, 4, 10)


def _narrow_solid():
    """Ordinary terrain, a 2 x 2 x 2 block floating above it and a one-voxel cavity inside a thick patch of ground."""
    x, y, z = np.meshgrid(*[np.arange(d) for d in NARROW], indexing="ij")
    solid = y < 3 + (x + z) % 3
    solid |= (x >= 8) & (x < 13) & (z >= 8) & (z < 13) & (y < 8)
    solid[CAVITY] = False
    solid[BLOCK] = True
    return solid


def _world(dims, solid):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), _colour(x, y, z), threads=4)


def _mask(box):
    m = np.zeros(NARROW, dtype=bool)
    m[box] = True
    return m


def test_a_world_narrower_than_the_rounding_rejects_every_column_edit():
    """levelCount 5 rounds to 32 columns, the world has 16: every call that edits columns fails with the one message of
    cvxi::RoundEditRectangle and changes nothing.  (All six levels are uploaded: stamp, pieces, settle and cavities lay the arena out before
    they reach the rectangle, and that needs them; LOD 0 is what the calls would have rewritten first.)"""
    solid = _narrow_solid()
    whole = ((0, 0, 0), NARROW)
    # the three facts the calls' work depends on, from the volume alone
    assert solid[:, 0, :].all() and not solid[:, 8:, :][~_mask(BLOCK)[:, 8:, :]].any()  # terrain in every column, nothing but the block above it
    pieces, summary, _ = piecesmodel.analyse(solid, *whole, piecesmodel.GROUND)
    assert summary["floatingPieces"] == 1 and summary["anchoredPieces"] == 1 and int(pieces[0]["voxels"]) == 8
    assert pieces[0]["min"].tolist() == [4, 20, 4] and not solid[4:6, 8:20, 4:6].any()  # ... with air below it: it would fall
    cavities, totals, _ = cavitymodel.analyse(solid, *whole)
    assert totals["selectedCavities"] == 1 and totals["selectedVoxels"] == 1 and cavities[0]["seed"].tolist() == list(CAVITY)

    ws = _world(NARROW, solid)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        uploaded = ws.storage(0).tobytes()
        assert ctx.read_level(0)[0] == uploaded
        stats = ctx.edit_stats()
        triangle = host.Mesh.from_arrays({"position": np.float32([[2, 30, 2], [12, 30, 3], [3, 30, 12]]), "rgba": [[200, 100, 50, 255]] * 3})
        dense = np.full((3, 3, 5), 0xFF102030, dtype=np.uint32)
        calls = {
            "brush": lambda: ctx.brush([{"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": (2, 30, 2), "b": (5, 34, 5), "argb": 0xFF00FF00}], 5),
            "copy": lambda: ctx.copy([_placement((0, 0, 0), (4, 6, 4), (9, 40, 2))], 5),
            "write_voxels": lambda: ctx.write_voxels((6, 40, 6), dense, level_count=5),
            "world_light": lambda: ctx.world_light(*whole, sun_dir=(1, 1, 0), sun_level=100, sun_range=10, sky_level=100, sky_range=4, level_count=5),
            "stamp_mesh": lambda: ctx.stamp_mesh(triangle, gpu.BRUSH_FILL, 5),
            "world_pieces": lambda: ctx.world_pieces(*whole, gpu.ANCHOR_GROUND, gpu.PIECES_REMOVE, 5),
            "world_settle": lambda: ctx.world_settle(*whole, gpu.ANCHOR_GROUND, level_count=5),
            "world_cavities": lambda: ctx.world_cavities(*whole, gpu.CAVITIES_FILL, argb=0xFF808080, level_count=5),
        }
        for name, call in calls.items():
            with pytest.raises(gpu.CvxError, match=r"narrower than 2\^levelCount"):
                call()
            assert ctx.read_level(0)[0] == uploaded, f"{name}: LOD 0 changed"
            _assert_levels(ctx, ws, ws, 5, f"after the rejected {name}")
            assert ctx.edit_stats() == stats, name
    finally:
        ctx.close()
        ws.close()


def test_a_dense_write_over_the_format_limits_is_rejected_whole():
    """A solid box 1 x 32768 x 1 makes one run of 32768 voxels (RLEColumn keeps lengths in shorts) in the world of
    tests/test_gpu_world_brush.py's and tests/test_gpu_world_copy.py's over-limit tests, the one world tall enough: CVX_ERR_CAPACITY from the
    pipeline's check behind the count kernel, and the level stays as it was."""
    dims = (32, 32768, 32)
    xs, zs = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    xs, zs = xs.ravel(), zs.ravel()
    ys = (xs * 7 + zs * 3) % 50
    ws = host.WorldSet.from_voxels(dims, xs.astype(np.int32), ys.astype(np.int32), zs.astype(np.int32), _colour(xs, ys, zs), threads=4)
    box = np.full((1, 1, 32768), 0xFF000000, dtype=np.uint32)
    assert box.shape[2] == dims[1] > 32767 and box.all()  # every voxel of the column set: one run, longer than a short holds
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        before = ctx.read_level(0)[0]
        assert before == ws.storage(0).tobytes()
        stats = ctx.edit_stats()
        with pytest.raises(gpu.CvxError, match=r"error -4: a written column would need .* a run longer than 32767 voxels"):
            ctx.write_voxels((3, 0, 3), box, level_count=5)
        assert ctx.read_level(0)[0] == before
        assert ctx.edit_stats() == stats
    finally:
        ctx.close()
        ws.close()
