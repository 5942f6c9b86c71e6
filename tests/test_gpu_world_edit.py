"""GPU: editing the device-resident world in place (cvx_world_set_columns, cvx_world_edit; World.SetVoxelColumn, World.cs:151-159).

World A is uploaded and drawn; B differs from A only inside aligned rectangles (a dug crater, a tower deeper than its colour block, columns of
more than three runs, emptied columns).  After B's rectangles are applied to A's context, the raybuffers must be bit-identical to a fresh context
with B uploaded and to the CPU oracle on B's blobs -- through both kernels, with LOD distances that send rays through every level 0..5."""
import numpy as np
import pytest

import oraclelib as O
import scenes
import waves
from cpuvox_amd import gpu, host

pytestmark = pytest.mark.gpu

CLEAR = 0xDEADBEEF
DIMS = (128, 64, 128)
W, H = 320, 200
BOTH_KERNELS = [("batch kernel", gpu.LATENCY_NEVER), ("latency kernel", gpu.LATENCY_ALWAYS)]
# (position as fraction of the world, euler degrees, LOD distances: None = the frame's own, else forced so that every level is reached)
FORCED_LODS = (6.0, 12.0, 20.0, 30.0, 44.0, 1e9)
POSES = [
    ((-0.15, 0.9, -0.12), (20.0, 45.0, 0.0), None),
    ((-0.15, 0.9, -0.12), (20.0, 45.0, 0.0), FORCED_LODS),
    ((0.5, 1.3, 0.45), (75.0, 10.0, 0.0), FORCED_LODS),
    ((1.1, 0.6, 0.6), (10.0, 260.0, 0.0), FORCED_LODS),
]


def _colour(x, y, z, salt=0):
    return (0xFF000000 | (((x * 2654435761 + y * 40503 + z * 2246822519 + salt * 97) >> 7) & 0xFFFFFF)).astype(np.uint32)


def _terrain():
    """A: rolling terrain with a floating slab over part of it (two-run columns)."""
    dx, dy, dz = DIMS
    x, y, z = np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij")
    h = 14 + (6 * np.sin(x / 9.0) + 5 * np.cos(z / 7.0)).astype(np.int64)
    solid = y < h
    solid |= (y >= 34) & (y < 38) & ((x // 16 + z // 16) % 3 == 0)
    return solid


def _voxels(solid, salt=None):
    x, y, z = np.nonzero(solid)
    c = _colour(x, y, z)
    if salt is not None:
        c = np.where(salt[x, y, z] != 0, _colour(x, y, z, salt[x, y, z]), c).astype(np.uint32)
    return x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), c


def _world(solid, salt=None):
    return host.WorldSet.from_voxels(DIMS, *_voxels(solid, salt), threads=4)


def _edited(solid, rect, kind=0):
    """B: A changed inside rect = (x0, z0, sx, sz) only."""
    s = solid.copy()
    salt = np.zeros(s.shape, dtype=np.int64)
    x0, z0, sx, sz = rect
    cx, cz = x0 + sx // 2, z0 + sz // 2
    x, y, z = np.meshgrid(np.arange(DIMS[0]), np.arange(DIMS[1]), np.arange(DIMS[2]), indexing="ij")
    inside = (x >= x0) & (x < x0 + sx) & (z >= z0) & (z < z0 + sz)
    # crater
    s &= ~(inside & ((x - cx) ** 2 + (z - cz) ** 2 < (sx // 3) ** 2) & (y > 6))
    # a tower deeper than any colour block around it, with its own colours
    tower = inside & (x >= x0 + 1 + kind % 3) & (x < x0 + 7 + kind % 3) & (z >= z0 + 2) & (z < z0 + 10) & (y < DIMS[1] - 2)
    s |= tower
    salt[tower] = 1 + kind
    # columns of many runs
    s |= inside & (x >= x0 + sx - 6) & (x < x0 + sx - 2) & (z >= z0 + 1) & (z < z0 + 5) & (y % 5 == 0) & (y < 50)
    # emptied columns
    s &= ~(inside & (x >= x0 + 2) & (x < x0 + 5) & (z >= z0 + sz - 5) & (z < z0 + sz - 2))
    return s, salt


def _frames(ws):
    out = []
    for frac, eul, lods in POSES:
        pos = [frac[i] * ws.dims[i] for i in range(3)]
        fr = scenes.make_frame(ws, W, H, pos, eul, lod_error=1.0)
        if lods is not None:
            for i, d in enumerate(lods):
                fr.camera.LODDistances[i] = d
        out.append(fr)
    return out


def _draw(ctx, fr, mode):
    ctx.set_latency_kernel(mode)
    ctx.clear_raybuffers(0, CLEAR)
    ctx.draw_segments(fr, 0)
    ctx.set_latency_kernel(gpu.LATENCY_AUTO)
    n_td, n_lr = scenes.used_rows(fr)
    return ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr]


def _context(ws):
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    ctx.set_resolution(W, H)
    return ctx


def _assert_same(label, a, b):
    for part, x, y in (("topdown", a[0], b[0]), ("leftright", a[1], b[1])):
        diff = x != y
        assert not diff.any(), f"{label}/{part}: {int(diff.sum())} of {diff.size} pixels differ"


def _check_world(ctx, ws_expected, frames, label, fresh=True):
    """ctx renders what the oracle renders on ws_expected (and what a fresh context of ws_expected renders), through both kernels -- and, as a
    third mode, the frames repeated into one launch of full 64-ray waves (tests/waves.py), every frame against the oracle."""
    ref = _context(ws_expected) if fresh else None
    visited = np.zeros(6, dtype=np.int64)
    oracles = []
    try:
        for k, fr in enumerate(frames):
            o_td, o_lr, cnt = O.draw_segments(ws_expected, fr, W, H, clear=CLEAR)
            oracles.append((o_td, o_lr))
            visited += np.array(cnt.lodVisits[:6])
            n_td, n_lr = scenes.used_rows(fr)
            for name, mode in BOTH_KERNELS:
                got = _draw(ctx, fr, mode)
                _assert_same(f"{label} frame {k} {name} vs oracle", got, (o_td[:n_td], o_lr[:n_lr]))
                if ref is not None:
                    _assert_same(f"{label} frame {k} {name} vs fresh upload", got, _draw(ref, fr, mode))
        waves.check_full_waves(ctx, frames, W, H, label, oracles=oracles)
    finally:
        if ref is not None:
            ref.close()
    return visited


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    return solid, _world(solid)


def test_set_columns_level_by_level(world_a):
    """cvx_world_set_columns on each level in turn, the caller supplying that level's columns of B: after level l the context renders the world
    whose levels 0..l are B's and the rest A's; after level 5 it renders B."""
    solid_a, ws_a = world_a
    rect = (32, 64, 32, 32)
    solid_b, salt = _edited(solid_a, rect)
    ws_b = _world(solid_b, salt)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        _check_world(ctx, ws_a, frames[:1], "A", fresh=False)
        for lod in range(6):
            r = [v >> lod for v in rect]
            blob, count = ws_b.extract_region(lod, *r)
            ctx.set_columns(lod, *r, blob, count)
            mixed = host.WorldSet.from_blobs(DIMS, [ws_b.storage(k) if k <= lod else ws_a.storage(k) for k in range(6)])
            visited = _check_world(ctx, mixed, frames, f"after level {lod}", fresh=lod == 5)
        assert (visited > 0).all(), f"the frames reach LOD visits {visited.tolist()}: every level must be drawn"
        used, abandoned, spare = ctx.edit_stats()
        assert spare > 0 and used > 0
    finally:
        ctx.close()


def test_edit_rebuilds_the_levels_above(world_a):
    """cvx_world_edit with levelCount 5: LOD 0 of the rectangle from the caller, LOD 1..5 built on the device -- the same as B's host-built levels."""
    solid_a, ws_a = world_a
    rect = (64, 32, 64, 32)
    solid_b, salt = _edited(solid_a, rect, kind=1)
    ws_b = _world(solid_b, salt)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        _check_world(ctx, ws_a, frames[:1], "A", fresh=False)
        blob, count = ws_b.extract_region(0, *rect)
        ms = ctx.edit(*rect, blob, count, 5)
        assert ms > 0.0
        _check_world(ctx, ws_b, frames, "edited")
    finally:
        ctx.close()


def test_many_edits_move_blocks_and_grow_the_arena(world_a):
    """Sixteen 32 x 32 edits in a row, each with a tower deeper than its colour blocks: blocks move to the tail, the headroom runs out and the
    arena grows; the world stays bit-identical and edit_stats reports what the moves left behind."""
    solid_a, ws_a = world_a
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    solid, salt = solid_a, np.zeros(solid_a.shape, dtype=np.int64)
    try:
        _check_world(ctx, ws_a, frames[:1], "A", fresh=False)
        spares, k = [], 0
        for x0 in range(0, 128, 32):
            for z0 in range(0, 128, 32):
                solid, s = _edited(solid, (x0, z0, 32, 32), kind=k)
                salt = np.where(s != 0, s, salt)
                blob, count = _world(solid, salt).extract_region(0, x0, z0, 32, 32)
                ctx.edit(x0, z0, 32, 32, blob, count, 5)
                spares.append(ctx.edit_stats()[2])
                k += 1
                if k == 8:
                    _check_world(ctx, _world(solid, salt), frames[2:3], "after 8 edits", fresh=False)
        used, abandoned, spare = ctx.edit_stats()
        assert abandoned > 0, "block moves leave their old places behind"
        assert any(b > a for a, b in zip(spares, spares[1:])), f"the headroom never grew: {spares}"
        _check_world(ctx, _world(solid, salt), frames, "after 16 edits")
        # a full upload reclaims everything
        ctx.upload_world(ws_a)
        _check_world(ctx, ws_a, frames[:1], "A again", fresh=False)
        assert ctx.edit_stats()[1:] == (0, 0)
    finally:
        ctx.close()


def test_rejected_edits_leave_the_world_alone(world_a):
    solid_a, ws_a = world_a
    frames = _frames(ws_a)[1:2]
    ctx = _context(ws_a)
    solid_b, salt = _edited(solid_a, (32, 32, 32, 32))
    ws_b = _world(solid_b, salt)
    try:
        before = [_draw(ctx, fr, gpu.LATENCY_NEVER) for fr in frames]
        blob, count = ws_b.extract_region(0, 32, 32, 32, 32)
        with pytest.raises(gpu.CvxError, match="aligned"):
            ctx.edit(16, 32, 32, 32, blob, count, 5)                 # misaligned for levelCount 5
        with pytest.raises(gpu.CvxError, match="outside"):
            ctx.edit(128, 32, 32, 32, blob, count, 5)                # outside the world
        with pytest.raises(gpu.CvxError, match="outside"):
            ctx.set_columns(3, 10, 10, 8, 8, blob, count)             # LOD 3 has 16 x 16 columns
        with pytest.raises(gpu.CvxError, match="columnCount"):
            ctx.edit(32, 32, 32, 32, blob, count - 1, 5)             # fewer headers than the rectangle
        bad = bytearray(blob)
        # the last column's first run one voxel longer: its runs no longer add up to the column height
        first = np.frombuffer(blob, dtype=np.int32, count=3 * count).reshape(count, 3)
        i = max(k for k in range(count) if first[k, 1] & 0xFFFF)
        at = count * 12 + 4 * (int(first[i, 0]) + 1)
        run = int.from_bytes(bad[at:at + 4], "little")
        bad[at:at + 4] = (run + (1 << 16)).to_bytes(4, "little")
        with pytest.raises(gpu.CvxError, match="add up"):
            ctx.edit(32, 32, 32, 32, bytes(bad), count, 5)
        after = [_draw(ctx, fr, gpu.LATENCY_NEVER) for fr in frames]
        for k, (a, b) in enumerate(zip(before, after)):
            _assert_same(f"frame {k} after the rejected edits", b, a)
        assert ctx.edit_stats()[1:] == (0, 0)
    finally:
        ctx.close()


def test_edit_is_ordered_on_the_stream(world_a):
    """An async draw, then an edit, then a draw: the first buffer shows A, the second B."""
    solid_a, ws_a = world_a
    rect = (64, 32, 32, 32)
    solid_b, salt = _edited(solid_a, rect, kind=2)
    ws_b = _world(solid_b, salt)
    fr = _frames(ws_a)[3]  # (the oracle: ~2 400 pixels change)
    n_td, n_lr = scenes.used_rows(fr)
    ctx = _context(ws_a)
    try:
        _draw(ctx, fr, gpu.LATENCY_NEVER)
        blob, count = ws_b.extract_region(0, *rect)
        ctx.set_latency_kernel(gpu.LATENCY_NEVER)
        ctx.clear_raybuffers(0, CLEAR)
        ctx.clear_raybuffers(1, CLEAR)
        ctx.draw_segments(fr, 0, gpu.DRAW_ASYNC)
        ctx.edit(*rect, blob, count, 5)
        ctx.draw_segments(fr, 1, gpu.DRAW_ASYNC)
        ctx.synchronize()
        first = (ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        second = (ctx.read_raybuffer(1, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(1, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        for ws, got, label in ((ws_a, first, "draw before the edit"), (ws_b, second, "draw after the edit")):
            o_td, o_lr, _ = O.draw_segments(ws, fr, W, H, clear=CLEAR)
            _assert_same(label, got, (o_td[:n_td], o_lr[:n_lr]))
        assert not all((a == b).all() for a, b in zip(first, second)), "the edit must be visible in this frame"
    finally:
        ctx.close()


def test_edit_before_the_first_draw(world_a):
    """The uploaded levels are still pending: the edit places them in the arena first."""
    solid_a, ws_a = world_a
    rect = (0, 96, 32, 32)
    solid_b, salt = _edited(solid_a, rect, kind=3)
    ws_b = _world(solid_b, salt)
    ctx = _context(ws_a)
    try:
        blob, count = ws_b.extract_region(0, *rect)
        ctx.edit(*rect, blob, count, 5)
        _check_world(ctx, ws_b, _frames(ws_a)[1:3], "edited before drawing")
    finally:
        ctx.close()


def test_edit_of_a_level_that_keeps_its_colours_column_after_column():
    """A sparse world of deep columns keeps its colours column after column (colorShift 2, cvx_device.h): replaced columns that fit go to their
    old place, the others to the tail."""
    dims = (64, 128, 64)
    rng = np.random.default_rng(7)
    solid = np.zeros((dims[0], dims[1], dims[2]), dtype=bool)
    for _ in range(60):
        x, z = rng.integers(0, 64, 2)
        lo = int(rng.integers(0, 40))
        solid[x, lo:lo + int(rng.integers(10, 80)), z] = True
    def world(s):
        x, y, z = np.nonzero(s)
        return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), _colour(x, y, z), threads=4)
    ws_a = world(solid)
    b = solid.copy()
    b[0:32, :, 0:32] = False
    for _ in range(12):
        x, z = rng.integers(0, 32, 2)
        lo = int(rng.integers(0, 20))
        b[x, lo:lo + int(rng.integers(5, 100)), z] = True
    ws_b = world(b)
    frames = []
    for pos, eul in (((32.3, 150.0, -20.2), (25.0, 10.0, 0.0)), ((32.3, 200.0, 32.2), (80.0, 30.0, 0.0))):
        fr = scenes.make_frame(ws_a, W, H, pos, eul)
        for i, d in enumerate(FORCED_LODS):
            fr.camera.LODDistances[i] = d
        frames.append(fr)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws_a)
        ctx.set_resolution(W, H)
        _check_world(ctx, ws_a, frames[:1], "A", fresh=False)
        blob, count = ws_b.extract_region(0, 0, 0, 32, 32)
        ctx.edit(0, 0, 32, 32, blob, count, 5)
        _check_world(ctx, ws_b, frames, "sparse edited")
    finally:
        ctx.close()
