"""GPU: stamping triangle meshes into the device-resident world (cvx_world_stamp_mesh).

- mill.obj stamped into an empty world reads back, level by level, byte-identical to host.WorldSet.from_obj and the committed fixtures.
- Stamps into the terrain world of tests/test_gpu_world_edit.py (FILL / CARVE / PAINT, coloured and textured meshes, parts outside the world,
  levelCount 5 / 3 / 0) equal a host rebuild of a dense numpy model fed by the triangle rule compiled for the host (tests/stampmodel.py): the
  read-back matches and renders are bit-identical through both kernels and against the CPU oracle.
- The per-triangle cap, many stamps in a row with compaction, stream ordering and rejected calls."""
import numpy as np
import pytest

import oraclelib as O
import scenes
import stampmodel
from cpuvox_amd import gpu, host
from test_gpu_world_edit import CLEAR, DIMS, H, W, _assert_same, _check_world, _colour, _context, _draw, _frames, _terrain

pytestmark = pytest.mark.gpu

FILL, CARVE, PAINT = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("stamp")
    return d, stampmodel.rules(d)


def _dense(solid):
    x, y, z = np.nonzero(solid)
    colour = np.zeros(solid.shape, dtype=np.uint32)
    colour[x, y, z] = _colour(x, y, z)
    return colour


def _world(solid, colour, dims=DIMS):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def _empty(dims):
    e = np.zeros(0, dtype=np.int32)
    return host.WorldSet.from_voxels(dims, e, e, e, np.zeros(0, dtype=np.uint32))


def _mixed(ws_new, ws_old, level_count):
    return host.WorldSet.from_blobs(DIMS, [ws_new.storage(k) if k <= level_count else ws_old.storage(k) for k in range(6)])


def _levels(ctx):
    return [ctx.read_level(k)[0] for k in range(6)]


@pytest.fixture(scope="module")
def world_a():
    solid = _terrain()
    colour = _dense(solid)
    return solid, colour, _world(solid, colour)


def _coloured_mesh(seed, count=40, outside=True):
    """Random coloured triangles over the terrain world, some reaching past its edges."""
    rng = np.random.default_rng(seed)
    lo, hi = (np.array([-20.0, -8.0, -20.0]), np.array([148.0, 70.0, 148.0])) if outside else (np.zeros(3), np.array([127.0, 63.0, 127.0]))
    centres = rng.uniform(lo, hi, size=(count, 3))
    pos = (centres[:, None, :] + rng.normal(0.0, 9.0, size=(count, 3, 3))).reshape(-1, 3).astype(np.float32)
    rgba = rng.integers(0, 256, size=(count * 3, 4)).astype(np.uint8)
    return host.Mesh.from_arrays({"position": pos, "rgba": rgba})


def _textured_mesh():
    """Two textured quads (material 0 with transparent texels, material 1 without a texture = white) and one triangle of a material index
    out of range."""
    rng = np.random.default_rng(7)
    tex = rng.integers(0, 256, size=(16, 8, 4)).astype(np.uint8)
    tex[..., 3] = np.where(rng.random((16, 8)) < 0.3, 200, 255)
    quad = np.float32([[10, 30, 10], [90, 30, 10], [90, 50, 100], [10, 50, 100]])
    quad2 = quad + np.float32([20, -12, 5])
    pos = np.concatenate([quad, quad2, np.float32([[40, 5, 40], [120, 40, 60], [60, 60, 120]])])
    uv = np.float32([[0, 0], [1, 0], [1, 1], [0, 1]] * 2 + [[0, 0], [1, 0], [0, 1]])
    mat = np.int32([0] * 4 + [1] * 4 + [300] * 3)  # (int8_t)300 = 44: out of range
    rgba = np.full((11, 4), 255, dtype=np.uint8)
    rgba[4:8, :3] = [[200, 40, 40], [40, 200, 40], [40, 40, 200], [90, 90, 90]]
    idx = np.int32([0, 1, 2, 0, 2, 3, 4, 5, 6, 4, 6, 7, 8, 9, 10])
    return host.Mesh.from_arrays({"position": pos, "rgba": rgba, "uv": uv, "material": mat}, idx, [tex, None])


@pytest.mark.parametrize("max_dimension", [256, 512])
def test_mill_into_an_empty_world_equals_the_host_build(work, max_dimension):
    d, rules = work
    obj = stampmodel.mill_obj(d)
    mesh = host.Mesh.from_obj(obj)
    dims = mesh.rescale(max_dimension)
    expected = host.WorldSet.from_obj(obj, max_dimension)
    golden = scenes.load_world(f"mill{max_dimension}")
    assert tuple(expected.dims) == tuple(dims) == tuple(golden.dims)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(_empty(dims))
        ms = ctx.stamp_mesh(mesh, FILL, 5)
        assert ms > 0.0
        for k, blob in enumerate(_levels(ctx)):
            assert blob == expected.storage(k).tobytes(), f"LOD {k} differs from WorldSet.from_obj"
            assert blob == golden.storage(k).tobytes(), f"LOD {k} differs from the fixture"
    finally:
        ctx.close()


CASES = [("coloured", FILL, 5), ("coloured", CARVE, 3), ("coloured", PAINT, 0), ("textured", FILL, 5), ("textured", PAINT, 3)]


@pytest.mark.parametrize("kind,op,level_count", CASES)
def test_stamp_equals_rebuild(work, world_a, kind, op, level_count):
    d, rules = work
    solid_a, colour_a, ws_a = world_a
    mesh = _coloured_mesh(11) if kind == "coloured" else _textured_mesh()
    x, y, z, argb = stampmodel.voxelise(rules, mesh, DIMS, d)
    assert len(x) > 0
    solid_b, colour_b = stampmodel.apply_stamp(solid_a.copy(), colour_a.copy(), x, y, z, argb, op)
    ws_b = _world(solid_b, colour_b)
    frames = _frames(ws_a)
    ctx = _context(ws_a)
    try:
        ms = ctx.stamp_mesh(mesh, op, level_count)
        assert ms > 0.0
        got, columns = ctx.read_region(0, 0, 0, DIMS[0], DIMS[2])
        want, want_columns = ws_b.extract_region(0, 0, 0, DIMS[0], DIMS[2])
        assert columns == want_columns and got == want, "LOD 0 read-back differs from the host rebuild"
        expected = _mixed(ws_b, ws_a, level_count)
        for k in range(6):
            assert ctx.read_level(k)[0] == expected.storage(k).tobytes(), f"LOD {k}"
        _check_world(ctx, expected, frames, f"{kind} op {op} levelCount {level_count}")
    finally:
        ctx.close()


def test_cap_triangle_gives_the_hosts_voxels(work):
    """One triangle over a 1024 x 1024 floor: ~524 000 hits, of which the first 262144 (x, z, y order) count."""
    d, rules = work
    dims = (1024, 32, 1024)
    mesh = host.Mesh.from_arrays({"position": np.float32([[0, 4, 0], [1024, 4, 0], [0, 4, 1024]]), "rgba": [[250, 10, 10, 255], [10, 250, 10, 255], [10, 10, 250, 255]]})
    x, y, z, argb = stampmodel.voxelise(rules, mesh, dims, d)
    assert len(x) == 262144
    expected = host.WorldSet.from_voxels(dims, x, y, z, argb)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(_empty(dims))
        ctx.stamp_mesh(mesh, FILL, 5)
        for k, blob in enumerate(_levels(ctx)):
            assert blob == expected.storage(k).tobytes(), f"LOD {k}"
    finally:
        ctx.close()


def test_repeated_stamps_grow_the_arena_and_compact(work, world_a):
    d, rules = work
    solid_a, colour_a, ws_a = world_a
    solid, colour = solid_a.copy(), colour_a.copy()
    ctx = _context(ws_a)
    try:
        used0 = ctx.edit_stats()[0]
        for k in range(24):
            mesh = _coloured_mesh(100 + k, count=6, outside=False)
            op = (FILL, FILL, CARVE, PAINT)[k % 4]
            x, y, z, argb = stampmodel.voxelise(rules, mesh, DIMS, d)
            stampmodel.apply_stamp(solid, colour, x, y, z, argb, op)
            ctx.stamp_mesh(mesh, op, 5)
        ws_b = _world(solid, colour)
        before = _levels(ctx)
        assert before == [ws_b.storage(k).tobytes() for k in range(6)]
        used, abandoned, _ = ctx.edit_stats()
        assert used > used0 and abandoned > 0
        reclaimed, _ = ctx.compact()
        assert reclaimed > 0
        assert _levels(ctx) == before
        _check_world(ctx, ws_b, _frames(ws_a)[:2], "stamped 24 times, compacted")
    finally:
        ctx.close()


def test_stamp_is_ordered_on_the_stream(work, world_a):
    d, rules = work
    solid_a, colour_a, ws_a = world_a
    # a slab high over the terrain at x, z in 30 .. 100
    pos = np.float32([[30, 60, 30], [100, 60, 30], [100, 60, 100], [30, 60, 100]])
    mesh = host.Mesh.from_arrays({"position": pos, "rgba": [[68, 85, 102, 255]] * 4}, [0, 1, 2, 0, 2, 3])
    x, y, z, argb = stampmodel.voxelise(rules, mesh, DIMS, d)
    solid_b, colour_b = stampmodel.apply_stamp(solid_a.copy(), colour_a.copy(), x, y, z, argb, FILL)
    ws_b = _world(solid_b, colour_b)
    fr = _frames(ws_a)[0]
    n_td, n_lr = scenes.used_rows(fr)
    ctx = _context(ws_a)
    try:
        _draw(ctx, fr, gpu.LATENCY_NEVER)
        ctx.set_latency_kernel(gpu.LATENCY_NEVER)
        ctx.clear_raybuffers(0, CLEAR)
        ctx.clear_raybuffers(1, CLEAR)
        ctx.draw_segments(fr, 0, gpu.DRAW_ASYNC)
        ctx.stamp_mesh(mesh, FILL, 5)
        vox, face, hit_argb, t = ctx.pick(np.float32([[64.5, 63.9, 64.5]]), np.float32([[0, -1, 0]]), 100.0)
        ctx.draw_segments(fr, 1, gpu.DRAW_ASYNC)
        ctx.synchronize()
        assert vox[0].tolist() == [64, 60, 64] and hit_argb[0] == colour_b[64, 60, 64], (vox, hex(int(hit_argb[0])))
        first = (ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        second = (ctx.read_raybuffer(1, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(1, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        for ws, got, label in ((ws_a, first, "draw before the stamp"), (ws_b, second, "draw after the stamp")):
            o_td, o_lr, _ = O.draw_segments(ws, fr, W, H, clear=CLEAR)
            _assert_same(label, got, (o_td[:n_td], o_lr[:n_lr]))
    finally:
        ctx.close()


def test_rejected_stamps_leave_the_world_alone(world_a):
    solid_a, colour_a, ws_a = world_a
    ctx = _context(ws_a)
    try:
        ctx.stamp_mesh(_coloured_mesh(3, count=4, outside=False), FILL, 5)  # an edited world
        before, stats = _levels(ctx), ctx.edit_stats()
        good = {"position": np.float32([[10, 10, 10], [40, 10, 10], [10, 10, 40]])}
        bad_meshes = [
            (host.Mesh.from_arrays({"position": np.float32([[10, np.nan, 10], [40, 10, 10], [10, 10, 40]])}), FILL, 5, "not finite"),
            (host.Mesh.from_arrays({"position": np.float32([[10, 10, 10], [4e7, 10, 10], [10, 10, 40]])}), FILL, 5, "above 2"),
            (host.Mesh.from_arrays(good), 3, 5, "bad op"),
            (host.Mesh.from_arrays(good), FILL, 6, "levelCount"),
            (host.Mesh.from_arrays(good), FILL, -1, "levelCount"),
            (host.Mesh.from_arrays(good, textures=[None] * 129), FILL, 5, "materialCount"),
        ]
        for mesh, op, level_count, match in bad_meshes:
            with pytest.raises(gpu.CvxError, match=match):
                ctx.stamp_mesh(mesh, op, level_count)
        # indices: out of range, not a multiple of 3 (the raw call; host.Mesh refuses to hold such meshes)
        v = np.zeros(3, dtype=gpu.MESH_VERTEX_DTYPE)
        v["position"] = good["position"]
        for idx, match in ((np.int32([0, 1, 3]), "index"), (np.int32([0, 1]), "multiple of 3")):
            rc = gpu.lib().cvx_world_stamp_mesh(ctx._h, v.ctypes.data, 3, idx.ctypes.data, idx.size, None, 0, FILL, 5, None)
            assert rc == -1 and match in gpu.lib().cvx_last_error(ctx._h).decode()
        tex = np.zeros(4, dtype=np.uint8)
        table = (gpu._TextureStruct * 1)()
        table[0].width, table[0].height, table[0].rgba = 0, 1, tex.ctypes.data
        rc = gpu.lib().cvx_world_stamp_mesh(ctx._h, v.ctypes.data, 3, np.int32([0, 1, 2]).ctypes.data, 3, gpu.C.cast(table, gpu.C.c_void_p), 1, FILL, 5, None)
        assert rc == -1 and "texture" in gpu.lib().cvx_last_error(ctx._h).decode()
        assert _levels(ctx) == before and ctx.edit_stats() == stats
        # a mesh entirely outside the world stamps nothing
        outside = host.Mesh.from_arrays({"position": np.float32([[300, 10, 300], [340, 10, 300], [300, 10, 340]])})
        assert ctx.stamp_mesh(outside, FILL, 5) == 0.0
        assert _levels(ctx) == before
    finally:
        ctx.close()
