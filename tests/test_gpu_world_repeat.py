"""GPU: repeating worlds (cvx_set_world_repeat).  The oracle knows only the bounded world, so the check is an exact equivalence: rendering the
repeating world W gives the pixels of the bounded world T = W laid out k x k times (k a power of two), with the camera at the same float position
inside T and far enough from T's edge that no ray reaches it before the far clip.  Every float operation is then the same and every column lookup
returns the same data (T's level l is W's level l tiled: tests/test_world_repeat_cpu.py).  T itself is checked against the CPU oracle."""
import numpy as np
import pytest

import oraclelib as O
import repeatworld as R
import scenes
import waves
from cpuvox_amd import gpu, host

pytestmark = pytest.mark.gpu

W, H = 320, 240
CLEAR = waves.CLEAR
# world -> (k, far clip; None = the reference's 10 x the tile's largest dimension)
WORLDS = {"stripes64x64x64": (32, None), "mill256": (8, 900.0), "proc256": (8, 900.0)}
# poses: (offset from T's centre as a fraction of the room the far clip leaves, height as a fraction of dimY, euler degrees, LOD error)
POSES = [
    ((0.37, -0.21), 0.3, (6.0, 37.0, 0.0), 1.0),    # low over the ground, across many seams
    ((0.01, 0.013), 1.7, (84.0, 10.0, 0.0), 1.0),   # straight down on a seam corner (T's centre is a tile corner)
    ((-0.61, 0.93), 1.4, (25.0, 130.0, 0.0), 4.0),  # above the world top
    ((0.25, 0.5), 0.55, (0.0, 90.0, 0.0), 2.0),     # rays along an axis
    ((0.83, -0.11), 0.45, (3.0, 251.0, 0.0), 8.0),  # far clip over several periods at every level
]

_cache = {}


def _worlds(name):
    if name not in _cache:
        ws = scenes.load_world(name)
        k, far = WORLDS[name]
        _cache[name] = (ws, R.tile_world(ws, k), k, far)
    return _cache[name]


def _frames(name):
    ws, wt, k, far = _worlds(name)
    D = ws.dims[0]
    c = k * D / 2.0
    room = c - (10.0 * ws.max_dimension if far is None else far) - 33.0  # (the far clip plus one LOD-5 cell from T's edge)
    assert room > 0
    out = []
    for (ox, oz), fy, eul, err in POSES:
        fr = R.frame(ws, W, H, (c + ox * room, fy * ws.dims[1], c + oz * room), eul, far, err)
        assert fr.camera.FarClip + 32 <= c - max(abs(ox), abs(oz)) * room, "the camera is too close to T's edge"
        out.append(fr)
    return out


def _context(ws, repeat, buffer_count=2):
    ctx = gpu.Context(0, buffer_count=buffer_count)
    ctx.upload_world(ws)
    ctx.set_resolution(W, H)
    if repeat is not None:
        ctx.set_world_repeat(repeat)
    return ctx


def _draw(ctx, fr, mode, buffer=0):
    ctx.set_latency_kernel(mode)
    try:
        ctx.clear_raybuffers(buffer, CLEAR)
        ctx.draw_segments(fr, buffer)
    finally:
        ctx.set_latency_kernel(gpu.LATENCY_AUTO)
    return _read(ctx, fr, buffer)


def _read(ctx, fr, buffer):
    n_td, n_lr = scenes.used_rows(fr)
    return ctx.read_raybuffer(buffer, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(buffer, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr]


def _same(label, a, b):
    for part, x, y in zip(("topdown", "leftright"), a, b):
        diff = x != y
        if diff.any():
            r, p = np.nonzero(diff)
            raise AssertionError(f"{label}/{part}: {int(diff.sum())} of {diff.size} pixels differ, first at ray {r[0]} pixel {p[0]}: "
                                 f"{x[r[0], p[0]]:08x} vs {y[r[0], p[0]]:08x}")


def _mismatch(a, b):
    n = sum(x.size for x in a)
    return sum(int((x != y).sum()) for x, y in zip(a, b)) / max(n, 1)


@pytest.mark.parametrize("name", list(WORLDS))
def test_repeat_equals_tiled_bounded_world(name):
    ws, wt, k, far = _worlds(name)
    frames = _frames(name)
    cw, ct = _context(ws, True), _context(wt, None)
    try:
        sky = 0
        for i, fr in enumerate(frames):
            for mode, kernel in ((gpu.LATENCY_ALWAYS, "latency"), (gpu.LATENCY_NEVER, "batch")):
                want = _draw(ct, fr, mode)
                got = _draw(cw, fr, mode)
                _same(f"{name} pose {i} {kernel} kernel", got, want)
                sky += int((want[0] == 0x191919FF).sum())
            # the counting build: pixels and every counter
            for c in (cw, ct):
                c.enable_counters(True)
            try:
                want, got = _draw(ct, fr, gpu.LATENCY_NEVER), _draw(cw, fr, gpu.LATENCY_NEVER)
                cnt_t, cnt_w = ct.counters().as_dict(), cw.counters().as_dict()
            finally:
                for c in (cw, ct):
                    c.enable_counters(False)
            _same(f"{name} pose {i} counting build", got, want)
            assert cnt_w == cnt_t, (name, i, cnt_w, cnt_t)
        # the same world rendered bounded (a fresh context) differs: the repeat path is what the comparison above exercised
        cb = _context(ws, None)
        try:
            assert any(_mismatch(_draw(cb, fr, gpu.LATENCY_NEVER), _draw(cw, fr, gpu.LATENCY_NEVER)) > 0 for fr in frames)
        finally:
            cb.close()
    finally:
        cw.close()
        ct.close()


@pytest.mark.parametrize("name", ["stripes64x64x64", "mill256"])
def test_repeat_batched_draws_and_full_waves(name):
    ws, wt, k, far = _worlds(name)
    frames = _frames(name)
    n = len(frames)
    cw, ct = _context(ws, True, n), _context(wt, None, n)
    try:
        for mode in (gpu.LATENCY_ALWAYS, gpu.LATENCY_NEVER):
            res = []
            for c in (cw, ct):
                c.set_latency_kernel(mode)
                for b in range(n):
                    c.clear_raybuffers(b, CLEAR)
                c.draw_segments_batch(frames, 0)
                c.set_latency_kernel(gpu.LATENCY_AUTO)
                res.append([_read(c, fr, b) for b, fr in enumerate(frames)])
            for b in range(n):
                _same(f"{name} batch of {n}, mode {mode}, frame {b}", res[0][b], res[1][b])
        # full 64-ray waves of the batch kernel (tests/waves.py), against bounded(T) in place of the oracle (its rays used rows of each frame)
        oracles = [_draw(ct, fr, gpu.LATENCY_NEVER) for fr in frames]
        waves.check_full_waves(cw, frames, W, H, f"{name} repeat", oracles=oracles)
    finally:
        cw.close()
        ct.close()


def test_tiled_world_is_the_oracles():
    """The chain's other link: bounded(T) against the CPU oracle, for two small frames."""
    ws, wt, k, far = _worlds("stripes64x64x64")
    frames = _frames("stripes64x64x64")
    ct = _context(wt, None)
    try:
        for i in (0, 4):
            o_td, o_lr, _ = O.draw_segments(wt, frames[i], W, H, clear=CLEAR, counters=False)
            n_td, n_lr = scenes.used_rows(frames[i])
            _same(f"T pose {i} vs oracle", _draw(ct, frames[i], gpu.LATENCY_NEVER), (o_td[:n_td], o_lr[:n_lr]))
    finally:
        ct.close()


def test_negative_coordinates_wrap():
    ws, wt, k, far = _worlds("proc256")
    D = ws.dims[0]
    cw, ct_rep, ct = _context(ws, True), _context(wt, True), _context(wt, None)
    fractions = []
    try:
        for (px, pz), eul in (((5.25, 7.5), (8.0, 225.0, 0.0)), ((40.5, 3.75), (15.0, 180.0, 0.0)), ((2.5, 90.25), (5.0, 270.0, 0.0))):
            fr = R.frame(ws, W, H, (px, 0.4 * ws.dims[1], pz), eul, far, 2.0)
            m = k // 2
            fr_t = R.frame(ws, W, H, (px + m * D, 0.4 * ws.dims[1], pz + m * D), eul, far, 2.0)
            for mode in (gpu.LATENCY_ALWAYS, gpu.LATENCY_NEVER):
                got = _draw(cw, fr, mode)
                _same(f"repeat(W) vs repeat(T) at ({px}, {pz}) mode {mode}", got, _draw(ct_rep, fr, mode))
                fractions.append(_mismatch(got, _draw(ct, fr_t, mode)))
        print("negative-coordinate mismatch fractions against bounded(T) at +m*D:", fractions)
        # (measured on the MI355X: at most 1.3e-4 of the pixels, from the different rounding of the shifted float position)
        assert max(fractions) < 1e-3, fractions
    finally:
        for c in (cw, ct_rep, ct):
            c.close()


def _host_picks(tmp_path, ws, rays):
    """Bounded picks with the host build of PickRay (tests/brush_rules.cpp, the harness of tests/test_world_brush_cpu.py)."""
    import subprocess
    import ruleslib
    exe = ruleslib.build("brush_rules", tmp_path)
    blob, rays_in, hits_out = tmp_path / "blob.bin", tmp_path / "rays.bin", tmp_path / "hits.bin"
    np.array(ws.storage(0)).tofile(blob)
    rays.tofile(rays_in)
    info = ws.info(0)
    subprocess.check_output([exe, "pick", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(rays_in), str(hits_out)])
    return np.fromfile(hits_out, dtype=gpu.PICK_HIT_DTYPE)


def test_picks_wrap(tmp_path):
    ws, wt, k, far = _worlds("mill256")
    D = ws.dims[0]
    cw = _context(ws, True)
    rng = np.random.default_rng(7)
    try:
        n = 4096
        c = k * D / 2.0
        o = np.stack([c + rng.uniform(-1.5, 1.5, n) * D, rng.uniform(0, 1.3, n) * ws.dims[1], c + rng.uniform(-1.5, 1.5, n) * D], 1).astype(np.float32)
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d[:, 1] = -np.abs(d[:, 1]) * 0.3
        d /= np.linalg.norm(d, axis=1, keepdims=True)  # (unit directions: no ray gets within 300 voxels of T's edge)
        rays = np.zeros(n, dtype=gpu.PICK_RAY_DTYPE)
        rays["origin"], rays["direction"], rays["maxT"] = o, d, 300.0
        want = _host_picks(tmp_path, wt, rays)  # bounded picks on T
        got = cw.pick(o, d, 300.0)
        hit = want["face"] >= 0
        assert hit.sum() > n // 20  # (the mill is a sparse model: ~40 % of these rays hit)
        assert np.array_equal(got[1], want["face"]) and np.array_equal(got[2], want["argb"]) and np.array_equal(got[3], want["t"])
        assert np.array_equal(got[0][hit], want["voxel"][hit] % np.array([D, 1 << 30, D])), "voxel mod D"
        # rays heading toward negative coordinates report voxels inside [0, D)
        o2 = np.stack([rng.uniform(0, 8, n), rng.uniform(0, 1.2, n) * ws.dims[1], rng.uniform(0, 8, n)], 1).astype(np.float32)
        d2 = np.stack([-rng.uniform(0.2, 1, n), -rng.uniform(0.05, 0.4, n), -rng.uniform(0.2, 1, n)], 1).astype(np.float32)
        v, f, a, t = cw.pick(o2, d2, 500.0)
        h2 = f >= 0
        assert h2.sum() > n // 20
        assert (v[h2][:, [0, 2]] >= 0).all() and (v[h2][:, [0, 2]] < D).all()
    finally:
        cw.close()


def test_brush_then_render():
    ws, wt, k, far = _worlds("proc256")
    cw = _context(ws, True)
    frames = _frames("proc256")
    try:
        cw.brush([{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_SPHERE, "a": (250, 120, 5), "radius": 40, "argb": 0},
                  {"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": (0, 100, 200), "b": (30, 160, 256), "argb": 0xFF3366CC}])
        edited = cw.download()
        ct = _context(R.tile_world(edited, k), None)
        try:
            for i, fr in enumerate(frames[:3]):
                for mode in (gpu.LATENCY_ALWAYS, gpu.LATENCY_NEVER):
                    _same(f"brushed pose {i} mode {mode}", _draw(cw, fr, mode), _draw(ct, fr, mode))
        finally:
            ct.close()
    finally:
        cw.close()


def test_rejections_and_default():
    ws = scenes.load_world("proc256")
    fr = _frames("proc256")[0]
    ctx = _context(ws, None)
    try:
        for bad in (2, -1, 7):
            assert gpu.lib().cvx_set_world_repeat(ctx._h, bad) != 0
        bounded = _draw(ctx, fr, gpu.LATENCY_NEVER)  # a fresh context renders bounded: equal to a context set back to 0
        ctx.set_world_repeat(True)
        ctx.set_world_repeat(False)
        _same("set back to bounded", _draw(ctx, fr, gpu.LATENCY_NEVER), bounded)
        ctx.set_world_repeat(True)
        big = R.frame(ws, W, H, (100.0, 50.0, 100.0), (10.0, 20.0, 0.0), 2.0 ** 20 * 1.5)
        with pytest.raises(gpu.CvxError, match="FarClip"):
            ctx.draw_segments(big, 0)
        with pytest.raises(gpu.CvxError, match="maxT"):
            ctx.pick([[1.0, 50.0, 1.0]], [[1.0, -0.1, 0.0]], 2.0 ** 21)
    finally:
        ctx.close()
    x, y, z = np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij")
    s = y < 4
    small = host.WorldSet.from_voxels((16, 16, 16), x[s].astype(np.int32), y[s].astype(np.int32), z[s].astype(np.int32),
                                      np.full(int(s.sum()), 0xFF2040FF, np.uint32))
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(small)
        ctx.set_resolution(W, H)
        fr = R.frame(small, W, H, (8.0, 10.0, 8.0), (10.0, 20.0, 0.0), None)
        ctx.draw_segments(fr, 0)  # bounded: fine
        ctx.set_world_repeat(True)
        with pytest.raises(gpu.CvxError, match="at least 32"):
            ctx.draw_segments(fr, 0)
        with pytest.raises(gpu.CvxError, match="at least 32"):
            ctx.pick([[1.0, 10.0, 1.0]], [[1.0, -0.1, 0.0]], 10.0)
    finally:
        ctx.close()
