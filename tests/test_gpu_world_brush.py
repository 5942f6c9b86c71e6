"""GPU: voxel brushes (cvx_world_brush) and ray picking (cvx_world_pick) on the device-resident world.

Brushes: the strokes are applied to world A's context and, independently, to A's dense numpy volume, from which B is built on the host
(host.WorldSet.from_voxels).  The context must then render bit-identically to a fresh upload of B and to the CPU oracle on B's blobs, through
both kernels, with LOD distances that send rays through every level (the world and poses of tests/test_gpu_world_edit.py).
Picks: against the float64 dense model of tests/pickmodel.py, exact on every ray it calls unambiguous, before and after brushes."""
import numpy as np
import pytest

import oraclelib as O
import pickmodel
import scenes
from cpuvox_amd import gpu, host
from test_gpu_world_edit import CLEAR, DIMS, FORCED_LODS, H, W, _assert_same, _check_world, _colour, _context, _draw, _frames, _terrain

pytestmark = pytest.mark.gpu

FILL, CARVE, PAINT = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT
BOX, SPHERE = gpu.SHAPE_BOX, gpu.SHAPE_SPHERE


def _box(op, a, b, argb=0):
    return {"op": op, "shape": BOX, "a": a, "b": b, "argb": argb}


def _sphere(op, c, r, argb=0):
    return {"op": op, "shape": SPHERE, "a": c, "radius": r, "argb": argb}


def _dense(solid):
    x, y, z = np.nonzero(solid)
    colour = np.zeros(solid.shape, dtype=np.uint32)
    colour[x, y, z] = _colour(x, y, z)
    return colour


def _world(solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(DIMS, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def _brushed(solid, colour, strokes):
    s, c = solid.copy(), colour.copy()
    pickmodel.apply_strokes(s, c, gpu.strokes_array(strokes))
    return s, c


def _mixed(ws_new, ws_old, level_count):
    """What a context shows after a brush with level_count: LOD 0..level_count refreshed, the levels above as they were."""
    return host.WorldSet.from_blobs(DIMS, [ws_new.storage(k) if k <= level_count else ws_old.storage(k) for k in range(6)])


def _hits(result):
    vox, face, argb, t = result
    out = np.zeros(len(face), dtype=gpu.PICK_HIT_DTYPE)
    out["voxel"], out["face"], out["argb"], out["t"] = vox, face, argb, t
    return out


# the stroke list of the rebuild test: every kind of change, footprints that are not aligned to 32 columns
STROKES = [
    _sphere(CARVE, (40, 6, 44), 12),                            # a crater reaching the bottom: columns emptied
    _box(FILL, (70, 0, 20), (76, 60, 27), 0xFF2040F0),          # a tower deeper than its colour blocks
    _box(FILL, (84, 44, 70), (101, 47, 90), 0xFFA0A000),        # a floating slab over the terrain and the slabs: 3 solid runs
    _box(FILL, (90, 52, 75), (95, 53, 80), 0xFF00FFFF),         # ... and a fourth above it
    _sphere(PAINT, (60, 20, 60), 9, 0xFF808080),                # paint over a mixed region (air stays air)
    _box(FILL, (20, 18, 90), (30, 30, 100), 0xFF0000FF),        # order matters: fill, carve inside it, fill part of the hole again,
    _sphere(CARVE, (25, 24, 95), 4),                            #   paint the whole box
    _box(FILL, (24, 22, 93), (26, 24, 97), 0xFF00FF00),
    _box(PAINT, (20, 18, 90), (30, 30, 100), 0xFFFF00FF),
    _sphere(FILL, (126, 50, 3), 6, 0xFF123456),                 # clipped by the world's edge
    _box(CARVE, (200, 0, 0), (300, 10, 10)),                    # entirely outside: does nothing
]


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    colour = _dense(solid)
    return solid, colour, _world(solid, colour)


@pytest.mark.parametrize("level_count", [5, 3, 0])
def test_brush_equals_rebuild(world_a, level_count):
    solid_a, colour_a, ws_a = world_a
    solid_b, colour_b = _brushed(solid_a, colour_a, STROKES)
    ws_b = _world(solid_b, colour_b)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        _check_world(ctx, ws_a, frames[:1], "A", fresh=False)
        ms = ctx.brush(STROKES, level_count)
        assert ms > 0.0
        visited = _check_world(ctx, _mixed(ws_b, ws_a, level_count), frames, f"brushed, levelCount {level_count}")
        assert (visited > 0).all(), f"the frames reach LOD visits {visited.tolist()}: every level must be drawn"
    finally:
        ctx.close()


def _tower_strokes(rng, count):
    out = []
    for k in range(count):
        x, z = int(rng.integers(0, 120)), int(rng.integers(0, 120))
        if k % 4 == 3:
            out.append(_sphere(CARVE, (x, int(rng.integers(5, 30)), z), int(rng.integers(3, 9))))
        else:  # towers with colours of their own: deeper than their blocks, which move to the tail
            out.append(_box(FILL, (x, 0, z), (x + int(rng.integers(2, 7)), int(rng.integers(30, 64)), z + int(rng.integers(2, 9))),
                            int(rng.integers(0, 2**32))))
    return out


def test_repeated_strokes_equal_one_call_and_the_rebuild(world_a):
    """Sixty-four single-stroke calls move blocks to the tails and grow the arena; the world equals one call with all 64 strokes and B."""
    solid_a, colour_a, ws_a = world_a
    strokes = _tower_strokes(np.random.default_rng(64), 64)
    solid_b, colour_b = _brushed(solid_a, colour_a, strokes)
    ws_b = _world(solid_b, colour_b)
    frames = _frames(ws_a)
    one, many = _context(ws_a), _context(ws_a)
    try:
        _draw(many, frames[0], gpu.LATENCY_NEVER)
        spares = []
        for s in strokes:
            many.brush([s], 5)
            spares.append(many.edit_stats()[2])
        used, abandoned, spare = many.edit_stats()
        assert abandoned > 0, "block moves leave their old places behind"
        assert any(b > a for a, b in zip(spares, spares[1:])), f"the headroom never grew: {spares}"
        one.brush(strokes, 5)
        _check_world(many, ws_b, frames, "64 calls")
        _check_world(one, ws_b, frames[1:3], "one call of 64 strokes", fresh=False)
        for fr in frames:
            for _, mode in (("batch", gpu.LATENCY_NEVER), ("latency", gpu.LATENCY_ALWAYS)):
                _assert_same("64 calls vs one call", _draw(many, fr, mode), _draw(one, fr, mode))
    finally:
        one.close()
        many.close()


def _check_picks(ctx, solid, colour, rng, n, label):
    o, d, max_t = pickmodel.random_rays(rng, DIMS, n)
    got = _hits(ctx.pick(o, d, max_t))
    model = pickmodel.pick_many(solid, colour, o, d, max_t)
    fraction = pickmodel.compare_picks(got, model, label)
    assert fraction >= 0.99, f"{label}: only {fraction:.4f} of the rays are unambiguous"
    hit = got["face"] >= 0
    assert (got["argb"][hit] == colour[tuple(got["voxel"][hit].T)]).all(), "the hit colour is the voxel's"
    return got, model


def test_pick_matches_the_model_before_and_after_a_brush(world_a):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    rng = np.random.default_rng(5)
    try:
        got, model = _check_picks(ctx, solid_a, colour_a, rng, 4096, "A")
        faces = model[1]
        assert all((faces == f).sum() > 5 for f in range(-1, 7)), np.bincount(faces + 1)
        # after brushes that move blocks to the tail and make listed columns
        strokes = STROKES + _tower_strokes(np.random.default_rng(9), 16)
        for s in strokes:
            ctx.brush([s], 5)
        assert ctx.edit_stats()[1] > 0
        solid_b, colour_b = _brushed(solid_a, colour_a, strokes)
        _check_picks(ctx, solid_b, colour_b, rng, 4096, "brushed")
        # straight down the columns of the four-run slab, and along its column boundaries
        xs, zs = np.meshgrid(np.arange(84, 101), np.arange(70, 90), indexing="ij")
        o = np.stack([xs.ravel() + 0.5, np.full(xs.size, 63.9), zs.ravel() + 0.25], axis=1).astype(np.float32)
        o = np.concatenate([o, o - np.float32([0.5, 0.0, 0.25])])
        d = np.tile(np.float32([0.0, -1.0, 0.0]), (len(o), 1))
        got = _hits(ctx.pick(o, d, 100.0))
        model = pickmodel.pick_many(solid_b, colour_b, o, d, 100.0)
        assert pickmodel.compare_picks(got, model, "down the slab") == 1.0
    finally:
        ctx.close()


def test_a_million_rays_agree_with_a_subset(world_a):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    rng = np.random.default_rng(11)
    try:
        n = 1 << 20
        dims = np.array(DIMS, dtype=np.float32)
        o = (rng.uniform(-0.3, 1.3, size=(n, 3)) * dims).astype(np.float32)
        d = (rng.uniform(0.0, 1.0, size=(n, 3)) * dims - o).astype(np.float32)
        d[np.all(d == 0.0, axis=1)] = (0.0, -1.0, 0.0)
        full = _hits(ctx.pick(o, d, 1e4))
        pick = rng.choice(n, size=4096, replace=False)
        part = _hits(ctx.pick(o[pick], d[pick], 1e4))
        assert (full[pick].tobytes() == part.tobytes()), "a ray's hit depends on its batch"
        assert 0.2 < (full["face"] >= 0).mean() < 0.99
    finally:
        ctx.close()


def test_pick_and_draws_are_ordered_with_the_brush(world_a):
    """An async draw, a brush, a pick and another async draw: the first draw shows A, the pick and the second draw the brushed world."""
    solid_a, colour_a, ws_a = world_a
    strokes = [_sphere(CARVE, (64, 20, 64), 14), _box(FILL, (30, 0, 30), (40, 60, 40), 0xFF445566)]
    solid_b, colour_b = _brushed(solid_a, colour_a, strokes)
    ws_b = _world(solid_b, colour_b)
    fr = _frames(ws_a)[2]
    n_td, n_lr = scenes.used_rows(fr)
    ctx = _context(ws_a)
    try:
        _draw(ctx, fr, gpu.LATENCY_NEVER)
        ctx.set_latency_kernel(gpu.LATENCY_NEVER)
        ctx.clear_raybuffers(0, CLEAR)
        ctx.clear_raybuffers(1, CLEAR)
        ctx.draw_segments(fr, 0, gpu.DRAW_ASYNC)
        ctx.brush(strokes, 5)
        o = np.float32([[64.5, 63.5, 64.5], [35.5, 63.5, 35.5]])
        vox, face, argb, t = ctx.pick(o, np.float32([[0, -1, 0], [0, -1, 0]]), 100.0)
        ctx.draw_segments(fr, 1, gpu.DRAW_ASYNC)
        ctx.synchronize()
        assert vox[1].tolist() == [35, 59, 35] and argb[1] == 0xFF445566, (vox, argb)
        assert vox[0][1] < 6 or face[0] == -1, "the crater is seen by the pick"
        first = (ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        second = (ctx.read_raybuffer(1, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(1, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        for ws, got, label in ((ws_a, first, "draw before the brush"), (ws_b, second, "draw after the brush")):
            o_td, o_lr, _ = O.draw_segments(ws, fr, W, H, clear=CLEAR)
            _assert_same(label, got, (o_td[:n_td], o_lr[:n_lr]))
        assert not all((a == b).all() for a, b in zip(first, second)), "the brush must be visible in this frame"
    finally:
        ctx.close()


def test_rejected_brushes_leave_the_world_alone(world_a):
    solid_a, colour_a, ws_a = world_a
    frames = _frames(ws_a)[1:2]
    ctx = _context(ws_a)
    try:
        before = [_draw(ctx, fr, gpu.LATENCY_NEVER) for fr in frames]
        good = _sphere(CARVE, (64, 20, 64), 10)
        for bad, match in ((dict(good, op=7), "bad op"), (dict(good, shape=5), "bad shape"), (_sphere(FILL, (1, 1, 1), -2), "radius")):
            with pytest.raises(gpu.CvxError, match=match):
                ctx.brush([good, bad, good], 5)
        with pytest.raises(gpu.CvxError, match="levelCount"):
            ctx.brush([good], 6)
        with pytest.raises(gpu.CvxError, match="strokeCount"):
            ctx.brush([good] * (gpu.BRUSH_MAX_STROKES + 1), 5)
        assert ctx.brush([_box(FILL, (-10, 0, 0), (-1, 10, 10))], 5) == 0.0  # outside the world: nothing to do
        after = [_draw(ctx, fr, gpu.LATENCY_NEVER) for fr in frames]
        for k, (a, b) in enumerate(zip(before, after)):
            _assert_same(f"frame {k} after the rejected brushes", b, a)
        assert ctx.edit_stats()[1:] == (0, 0)
    finally:
        ctx.close()


def test_a_brush_over_the_format_limits_is_rejected_whole():
    """A stroke in the middle of the list makes a run of 32768 voxels (RLEColumn keeps lengths in shorts): CVX_ERR_CAPACITY, and neither the
    strokes before it nor the ones after it change the world."""
    dims = (32, 32768, 32)
    xs, zs = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    xs, zs = xs.ravel(), zs.ravel()
    ys = (xs * 7 + zs * 3) % 50
    colour = _colour(xs, ys, zs)
    ws = host.WorldSet.from_voxels(dims, xs.astype(np.int32), ys.astype(np.int32), zs.astype(np.int32), colour, threads=4)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        o = np.stack([xs + 0.5, np.full(xs.size, 100.0), zs + 0.5], axis=1).astype(np.float32)
        d = np.tile(np.float32([0, -1, 0]), (len(o), 1))
        before = _hits(ctx.pick(o, d, 1000.0))
        assert (before["voxel"][:, 1] == ys).all() and (before["argb"] == colour).all()
        strokes = [_sphere(CARVE, (5, 10, 5), 6), _box(FILL, (3, 0, 3), (4, 32768, 4), 0xFF000000), _box(FILL, (10, 0, 10), (20, 80, 20), 0xFF0000FF)]
        with pytest.raises(gpu.CvxError, match="32767"):
            ctx.brush(strokes, 5)
        after = _hits(ctx.pick(o, d, 1000.0))
        assert after.tobytes() == before.tobytes()
        assert ctx.edit_stats()[1:] == (0, 0)
        ctx.brush(strokes[2:], 5)  # the last stroke alone is fine
        got = _hits(ctx.pick(o, d, 1000.0))
        inside = (xs >= 10) & (xs < 20) & (zs >= 10) & (zs < 20)
        assert (got["voxel"][inside, 1] == 79).all() and (got["voxel"][~inside, 1] == ys[~inside]).all()
    finally:
        ctx.close()
        ws.close()


def test_pick_screen_finds_the_voxel_under_each_pixel(world_a):
    """For a pose where every ray stays at LOD 0, the voxel pick_screen finds through a pixel's centre has the colour the blit shows at that
    pixel or at one of its 8 neighbours, for nearly every pixel (98 % on this pose, with the CPU oracle's screen too); at the pixel itself for
    about two thirds.  The renderer does not sample pixel centres: each ray of a segment fills the pixel rows between the integer-rounded
    projections of the column spans it crosses, and the blit takes every pixel from its nearest ray of the raybuffer (RayBufferBlit.shader), so
    along every voxel edge on screen the two disagree by up to a pixel (moving the pick half a pixel down changes the exact share from 64 % to
    74 %, no offset makes it exact)."""
    solid_a, colour_a, ws_a = world_a
    fr = scenes.make_frame(ws_a, W, H, [0.5 * DIMS[0], 40.0, 0.2 * DIMS[2]], (35.0, 20.0, 0.0), lod_error=1.0)
    for i in range(6):
        fr.camera.LODDistances[i] = 1e9
    ctx = _context(ws_a)
    try:
        ctx.draw_segments(fr, 0)
        screen = ctx.blit_segments(0)
        py, px = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        vox, face, argb, t = ctx.pick_screen(fr.camera, W, H, px.ravel(), py.ravel(), 1e4)
        hit = face >= 0
        exact = (argb == screen.ravel()) & hit
        near = np.zeros_like(hit)
        padded = np.pad(screen, 1, mode="edge")
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                near |= argb == padded[dy:dy + H, dx:dx + W].ravel()
        near &= hit
        f_exact, f_near = exact.sum() / max(1, hit.sum()), near.sum() / max(1, hit.sum())
        print(f"pick_screen: of {int(hit.sum())} hit pixels {f_exact:.4f} show the picked voxel's colour, {f_near:.4f} within one pixel")
        assert hit.mean() > 0.5 and f_near > 0.97 and f_exact > 0.55, (f_exact, f_near)
    finally:
        ctx.close()
