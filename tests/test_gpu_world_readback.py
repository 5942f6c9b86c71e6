"""GPU: reading the device-resident world back (cvx_world_read_region / cvx_world_read_level, Context.download) and compacting its arena
(cvx_world_compact).

Read-back: for every world the host library builds, a level read back is byte-identical to the blob that was uploaded, and a rectangle to
WorldSet.extract_region -- before any edit, and after brushes and edits against the host rebuild of the edited world.  A downloaded world saved,
loaded and uploaded again renders bit-identically to the edited context and to the CPU oracle; a rectangle read before a brush and written back
with edit() undoes it.  Compaction: renders, read-backs and picks are unchanged, the abandoned bytes are gone, later brushes still match the host
model.  The worlds, poses and helpers are those of tests/test_gpu_world_edit.py and tests/test_gpu_world_brush.py."""
import numpy as np
import pytest

import oraclelib as O
import scenes
from cpuvox_amd import gpu, host
from test_gpu_world_brush import CARVE, FILL, STROKES, _box, _brushed, _dense, _mixed, _sphere, _tower_strokes, _world
from test_gpu_world_edit import (BOTH_KERNELS, CLEAR, DIMS, FORCED_LODS, H, W, _assert_same, _check_world, _colour, _context, _draw, _edited,
                                 _frames, _terrain)
from test_gpu_world_edit import _world as _salted_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    colour = _dense(solid)
    return solid, colour, _world(solid, colour)


def _sparse_world():
    """The sparse world of deep columns of tests/test_gpu_world_edit.py: its levels keep their colours column after column (colorShift 2)."""
    dims = (64, 128, 64)
    rng = np.random.default_rng(7)
    solid = np.zeros(dims, dtype=bool)
    for _ in range(60):
        x, z = rng.integers(0, 64, 2)
        lo = int(rng.integers(0, 40))
        solid[x, lo:lo + int(rng.integers(10, 80)), z] = True
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), _colour(x, y, z), threads=4)


def _levels(ctx):
    return [ctx.read_level(k) for k in range(6)]


def _assert_levels(ctx, ws, label):
    for k in range(6):
        blob, count = ctx.read_level(k)
        assert count == ws.info(k).columnCount, f"{label} LOD {k}: {count} headers, want {ws.info(k).columnCount}"
        want = ws.storage(k).tobytes()
        assert blob == want, f"{label} LOD {k}: {len(blob)} bytes against {len(want)}, first difference at {_first_diff(blob, want)}"


def _first_diff(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return int(d[0]) if d.size else n


def _renders(ctx, frames):
    return [_draw(ctx, fr, mode) for fr in frames for _, mode in BOTH_KERNELS]


def _pick_rays(dims, n, seed):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-10, dims[0] + 10, n), rng.uniform(dims[1] * 0.6, dims[1] * 1.5, n), rng.uniform(-10, dims[2] + 10, n)], 1)
    d = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, -0.05, n), rng.uniform(-1, 1, n)], 1)
    return o.astype(np.float32), d.astype(np.float32)


# ---- read-back of unedited worlds ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["terrain", "sparse", "mill256"])
def test_read_back_of_an_uploaded_world_is_byte_identical(world_a, name):
    ws = world_a[2] if name == "terrain" else _sparse_world() if name == "sparse" else scenes.load_world("mill256")
    ctx = gpu.Context(0)
    rng = np.random.default_rng(11)
    try:
        ctx.upload_world(ws)  # (not drawn yet: the read-back places the levels first)
        _assert_levels(ctx, ws, name)
        for k in range(6):
            used_x, used_z = ws.dims[0] >> k, ws.dims[2] >> k
            for _ in range(6):
                sx, sz = int(rng.integers(1, used_x + 1)), int(rng.integers(1, used_z + 1))
                x0, z0 = int(rng.integers(0, used_x - sx + 1)), int(rng.integers(0, used_z - sz + 1))
                got = ctx.read_region(k, x0, z0, sx, sz)
                assert got == ws.extract_region(k, x0, z0, sx, sz), f"{name} LOD {k} rectangle {(x0, z0, sx, sz)}"
    finally:
        ctx.close()


# ---- read-back after brushes and edits -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("level_count", [5, 3, 0])
def test_read_back_after_brushes_equals_the_rebuild(world_a, level_count):
    solid_a, colour_a, ws_a = world_a
    ws_b = _world(*_brushed(solid_a, colour_a, STROKES))
    ctx = _context(ws_a)
    try:
        _draw(ctx, _frames(ws_a)[0], gpu.LATENCY_NEVER)
        ctx.brush(STROKES, level_count)
        _assert_levels(ctx, _mixed(ws_b, ws_a, level_count), f"brushed, levelCount {level_count}")
    finally:
        ctx.close()


def test_read_back_after_sixteen_edits_equals_the_rebuild(world_a):
    """The edit test's sequence: blocks move to the tails and the arena grows; read-back still gives the host build of the edited world."""
    solid = world_a[0]
    ws_a = _salted_world(solid)
    ctx = _context(ws_a)
    salt = np.zeros(solid.shape, dtype=np.int64)
    try:
        k = 0
        for x0 in range(0, 128, 32):
            for z0 in range(0, 128, 32):
                solid, s = _edited(solid, (x0, z0, 32, 32), kind=k)
                salt = np.where(s != 0, s, salt)
                blob, count = _salted_world(solid, salt).extract_region(0, x0, z0, 32, 32)
                ctx.edit(x0, z0, 32, 32, blob, count, 5)
                k += 1
        assert ctx.edit_stats()[1] > 0
        ws_b = _salted_world(solid, salt)
        _assert_levels(ctx, ws_b, "after 16 edits")
        assert ctx.read_region(0, 16, 40, 50, 33) == ws_b.extract_region(0, 16, 40, 50, 33)
        assert ctx.read_region(3, 2, 3, 9, 7) == ws_b.extract_region(3, 2, 3, 9, 7)
    finally:
        ctx.close()


def test_download_save_load_round_trip(world_a, tmp_path):
    solid_a, colour_a, ws_a = world_a
    strokes = STROKES + _tower_strokes(np.random.default_rng(5), 8)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        _draw(ctx, frames[0], gpu.LATENCY_NEVER)
        for s in strokes:
            ctx.brush([s], 5)
        saved = ctx.download()
        path = str(tmp_path / "edited.world")
        saved.save(path)
        loaded = host.WorldSet.load(path)
        _assert_levels(ctx, loaded, "loaded")
        # the reloaded world in a fresh context renders like the edited context, and like the oracle
        _check_world(ctx, loaded, frames, "saved and reloaded")
        _check_world(ctx, _world(*_brushed(solid_a, colour_a, strokes)), frames[1:2], "host model", fresh=False)
    finally:
        ctx.close()


def test_undo_by_writing_the_rectangle_back(world_a):
    solid_a, colour_a, ws_a = world_a
    strokes = [_sphere(CARVE, (40, 12, 44), 12), _box(FILL, (50, 0, 50), (58, 60, 60), 0xFF2040F0)]
    rect = (0, 32, 64, 32)  # (the strokes' footprints, rounded out to 2^5 columns)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        before = _renders(ctx, frames[1:3])
        blob, count = ctx.read_region(0, *rect)
        ctx.brush(strokes, 5)
        assert _levels(ctx)[0][0] != ws_a.storage(0).tobytes(), "the brush changes the world"
        ctx.edit(*rect, blob, count, 5)
        _assert_levels(ctx, ws_a, "undone")
        for got, want in zip(_renders(ctx, frames[1:3]), before):
            _assert_same("undone vs before the brush", got, want)
        _check_world(ctx, ws_a, frames[:1], "undone", fresh=False)
    finally:
        ctx.close()


# ---- compaction ------------------------------------------------------------------------------------------------------------------------------

def test_compact_after_many_brushes(world_a):
    solid_a, colour_a, ws_a = world_a
    strokes = _tower_strokes(np.random.default_rng(64), 64)
    frames = _frames(ws_a)
    o, d = _pick_rays(DIMS, 4096, 3)
    ctx = _context(ws_a)
    try:
        _draw(ctx, frames[0], gpu.LATENCY_NEVER)
        for s in strokes:
            ctx.brush([s], 5)
        used, abandoned, spare = ctx.edit_stats()
        assert abandoned > 0
        renders, levels, picks = _renders(ctx, frames), _levels(ctx), ctx.pick(o, d, 1e4)
        reclaimed, ms = ctx.compact()
        used2, abandoned2, spare2 = ctx.edit_stats()
        assert abandoned2 == 0
        assert used2 <= used - abandoned + 65536, (used, abandoned, used2)
        assert reclaimed == used - used2 and reclaimed >= abandoned - 65536 and ms > 0.0, (reclaimed, ms)
        for k, (got, want) in enumerate(zip(_renders(ctx, frames), renders)):
            _assert_same(f"compacted render {k}", got, want)
        assert _levels(ctx) == levels
        for got, want in zip(ctx.pick(o, d, 1e4), picks):
            assert (got == want).all()
        # nothing left to reclaim
        assert ctx.compact()[0] == 0
        assert ctx.edit_stats() == (used2, abandoned2, spare2)
        # the compacted arena takes further brushes (the headroom of a first edit, then growth)
        more = _tower_strokes(np.random.default_rng(65), 24)
        for s in more:
            ctx.brush([s], 5)
        ws_c = _world(*_brushed(solid_a, colour_a, strokes + more))
        _check_world(ctx, ws_c, frames, "brushed after the compaction")
        _assert_levels(ctx, ws_c, "brushed after the compaction")
    finally:
        ctx.close()


def test_compact_of_a_column_after_column_level():
    ws = _sparse_world()
    frames = []
    for pos, eul in (((32.3, 150.0, -20.2), (25.0, 10.0, 0.0)), ((32.3, 200.0, 32.2), (80.0, 30.0, 0.0))):
        fr = scenes.make_frame(ws, W, H, pos, eul)
        for i, dist in enumerate(FORCED_LODS):
            fr.camera.LODDistances[i] = dist
        frames.append(fr)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        ctx.set_resolution(W, H)
        for k in range(10):
            x, z = 5 + 6 * k, 60 - 6 * k
            ctx.brush([_box(FILL, (x, 0, z), (x + 2, 100 + k, z + 3), 0xFF000000 | (k * 0x10305)), _sphere(CARVE, (z, 30, x), 5)], 5)
        assert ctx.edit_stats()[1] > 0
        renders, levels = _renders(ctx, frames), _levels(ctx)
        reclaimed, _ = ctx.compact()
        assert reclaimed > 0 and ctx.edit_stats()[1] == 0
        for k, (got, want) in enumerate(zip(_renders(ctx, frames), renders)):
            _assert_same(f"compacted sparse render {k}", got, want)
        assert _levels(ctx) == levels
    finally:
        ctx.close()


def test_compact_of_a_context_that_never_edited(world_a):
    ws_a = world_a[2]
    frames = _frames(ws_a)[1:3]
    ctx = _context(ws_a)
    try:
        before = _renders(ctx, frames)
        stats = ctx.edit_stats()
        assert ctx.compact() == (0, 0.0)
        assert ctx.edit_stats() == stats
        for got, want in zip(_renders(ctx, frames), before):
            _assert_same("after a compaction that had nothing to do", got, want)
    finally:
        ctx.close()


def test_async_draw_before_compact_renders_the_world(world_a):
    solid_a, colour_a, ws_a = world_a
    strokes = _tower_strokes(np.random.default_rng(9), 16)
    ws_b = _world(*_brushed(solid_a, colour_a, strokes))
    fr = _frames(ws_a)[2]
    n_td, n_lr = scenes.used_rows(fr)
    ctx = _context(ws_a)
    try:
        _draw(ctx, fr, gpu.LATENCY_NEVER)
        for s in strokes:
            ctx.brush([s], 5)
        ctx.set_latency_kernel(gpu.LATENCY_NEVER)
        ctx.clear_raybuffers(0, CLEAR)
        ctx.clear_raybuffers(1, CLEAR)
        ctx.draw_segments(fr, 0, gpu.DRAW_ASYNC)
        assert ctx.compact()[0] > 0
        ctx.draw_segments(fr, 1, gpu.DRAW_ASYNC)
        ctx.synchronize()
        o_td, o_lr, _ = O.draw_segments(ws_b, fr, W, H, clear=CLEAR)
        for b in (0, 1):
            got = (ctx.read_raybuffer(b, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(b, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
            _assert_same(f"buffer {b}", got, (o_td[:n_td], o_lr[:n_lr]))
    finally:
        ctx.set_latency_kernel(gpu.LATENCY_AUTO)
        ctx.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------------

def test_read_back_errors_leave_the_world_alone(world_a):
    ws_a = world_a[2]
    ctx = gpu.Context(0)
    try:
        i = ws_a.info(0)
        assert gpu.lib().cvx_world_upload(ctx._h, 0, i.storage, i.byteLength, i.dimX, i.dimY, i.dimZ, i.columnCount) == 0
        with pytest.raises(gpu.CvxError, match="error -3"):
            ctx.read_level(3)  # never uploaded
        with pytest.raises(gpu.CvxError, match="error -3"):
            ctx.read_level(0)  # (the world is incomplete: nothing can be placed)
        ctx.upload_world(ws_a)
        ctx.brush(STROKES[:2], 5)
        levels, stats = _levels(ctx), ctx.edit_stats()
        for args in ((0, 120, 0, 16, 4), (0, -1, 0, 4, 4), (0, 0, 0, 0, 4), (5, 0, 0, 5, 1), (5, 3, 3, 1, 2), (6, 0, 0, 1, 1), (-1, 0, 0, 1, 1)):
            with pytest.raises(gpu.CvxError, match="error -1"):
                ctx.read_region(*args)
        with pytest.raises(gpu.CvxError, match="error -1"):
            ctx.read_level(6)
        assert _levels(ctx) == levels and ctx.edit_stats() == stats
    finally:
        ctx.close()


def test_read_back_is_ordered_after_a_brush_without_drawing(world_a):
    """read_region straight after brushes (no draw in between) sees them: the calls are ordered on the context's stream."""
    solid_a, colour_a, ws_a = world_a
    strokes = [_box(FILL, (8, 0, 8), (12, 63, 12), 0xFF0000FF)]
    ws_b = _world(*_brushed(solid_a, colour_a, strokes))
    ctx = _context(ws_a)
    try:
        ctx.brush(strokes, 0)
        assert ctx.read_region(0, 0, 0, 32, 32) == ws_b.extract_region(0, 0, 0, 32, 32)
    finally:
        ctx.close()
