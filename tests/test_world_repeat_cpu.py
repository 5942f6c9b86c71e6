"""Repeating worlds on the host side: cvxh_setup_lods_ex (UnityManager.SetupLods with the 10x far clip of World.REPEAT_WORLD), the tiled
world the GPU tests compare against, and the new exports and their argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import repeatworld as R
from cpuvox_amd import gpu, host

POSES = [((10.0, 40.0, 20.0), (10.0, 30.0, 0.0), 85.0), ((100.0, 5.0, 3.0), (-20.0, 200.0, 5.0), 60.0), ((0.0, 0.0, 0.0), (89.0, 0.0, 0.0), 100.0)]
RES = [(640, 480), (1920, 1080), (320, 240), (17, 9)]
ERRORS = [1.0, 4.0, 0.37]


def _raw(pose, dim, w, h, err, repeat=None):
    out = (C.c_float * host.LOD_LEVELS)()
    far = C.c_float()
    L = host.lib()
    rc = L.cvxh_setup_lods(C.byref(pose), dim, w, h, err, out, C.byref(far)) if repeat is None else \
        L.cvxh_setup_lods_ex(C.byref(pose), dim, w, h, err, repeat, out, C.byref(far))
    assert rc == 0
    return np.array(out, dtype=np.float32), np.float32(far.value)


def _setup_lods_model(fov_deg, pixel_w, pixel_h, dim, res_x, res_y, lod_error, clip_multiplier):
    """UnityManager.SetupLods (UnityManager.cs:417-458) in binary32 throughout (the `p += 0.0001f` loop is only bit-exact there)."""
    f = np.float32
    clip_max = f(dim * clip_multiplier)
    pw = f(f(1) / f(res_x)) * f(pixel_w)
    ph = f(f(1) / f(res_y)) * f(pixel_h)
    mw, mh = pixel_w // 2, pixel_h // 2
    aspect = f(pixel_w) / f(pixel_h)
    t = f(math.tan(f(f(fov_deg) * f(math.pi / 180.0)) * f(0.5)))

    def ray(px, py):
        nx = f(f(f(2) * f(px)) / f(pixel_w)) - f(1)
        ny = f(f(f(2) * f(py)) / f(pixel_h)) - f(1)
        v = np.array([f(f(nx * aspect) * t), f(ny * t), f(1)], dtype=np.float32)
        return v / np.float32(np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])))

    a, b = ray(f(mw), f(mh)), ray(f(mw) + pw, f(mh) + ph)
    have, lods = [False] * 6, [f(0)] * 6
    pixel_width = f(1.41) / f(lod_error)
    p = f(0)
    while p < f(1):
        dist = p * clip_max
        d = a * dist - b * dist
        pab = np.float32(np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
        for j in range(6):
            if not have[j] and pab > pixel_width * f(2 << j):
                have[j], lods[j] = True, p
        p = f(p + f(0.0001))
    have[5], lods[5] = True, f(2)
    return np.array([math.ceil(f((lods[i] if have[i] else f(2)) * clip_max)) for i in range(6)], dtype=np.float32), clip_max


def test_setup_lods_ex_bounded_is_setup_lods():
    for pos, eul, fov in POSES:
        for w, h in RES:
            for err in ERRORS:
                pose = host.camera_pose(pos, eul, w, h)
                pose.fieldOfView = fov
                for dim in (64, 256, 2048):
                    a, fa = _raw(pose, dim, w, h, err)
                    b, fb = _raw(pose, dim, w, h, err, repeat=0)
                    assert a.tobytes() == b.tobytes() and fa == fb and fa == 2 * dim
                    lods, far = host.setup_lods(pose, dim, w, h, err)
                    assert np.array(lods, dtype=np.float32).tobytes() == a.tobytes() and np.float32(far) == fa


def test_setup_lods_ex_repeat_is_the_reference_rule():
    checked = 0
    for pos, eul, fov in POSES[:2]:
        for w, h in RES[:3]:
            for err in ERRORS[:2]:
                pose = host.camera_pose(pos, eul, w, h)
                pose.fieldOfView = fov
                dim = 256
                got, far = _raw(pose, dim, w, h, err, repeat=1)
                want, clip = _setup_lods_model(fov, w, h, dim, w, h, err, 10)
                assert far == np.float32(10 * dim) == clip
                # (the model follows the reference's float32 arithmetic; the library's vector helpers may round a normalisation differently in the
                # last place, which moves a threshold by at most one 0.0001 step of p)
                step = np.float32(0.0001) * clip
                assert np.all(np.abs(got - want) <= np.ceil(step)), (pose, w, h, err, got, want)
                checked += int(np.array_equal(got, want))
                lods, far2 = host.setup_lods(pose, dim, w, h, err, repeat=True)
                assert np.array(lods, dtype=np.float32).tobytes() == got.tobytes() and np.float32(far2) == far
    assert checked >= 1


def test_tiled_world_levels_are_the_tile_levels_tiled():
    D, k = 64, 4
    x, y, z = np.meshgrid(np.arange(D), np.arange(D), np.arange(D), indexing="ij")
    h = (x * 73856093) ^ (z * 19349663)
    solid = (y < 8 + h % 23) | (((y + (h >> 5) % 7) % 9) < 2)  # a ground with floating bands: columns of several runs
    x, y, z = x[solid].astype(np.int32), y[solid].astype(np.int32), z[solid].astype(np.int32)
    argb = (0xFF000000 | ((x.astype(np.int64) * 2654435761 + y * 40503 + z * 97) & 0xFFFFFF)).astype(np.uint32)
    ws = host.WorldSet.from_voxels((D, D, D), x, y, z, argb, threads=4)
    xs = np.concatenate([x + i * D for i in range(k) for _ in range(k)])
    zs = np.concatenate([z + j * D for _ in range(k) for j in range(k)])
    big = host.WorldSet.from_voxels((D * k, ws.dims[1], D * k), xs, np.tile(y, k * k), zs, np.tile(argb, k * k), threads=4)
    tiled = R.tile_world(ws, k)
    assert tiled.dims == big.dims
    for lod in range(host.LOD_LEVELS):
        n = D >> lod
        sw, sb = R._split(ws, lod), R._split(big, lod)
        st = R._split(tiled, lod)
        for cx in range(0, n * k, max(1, n // 8)):
            for cz in range(0, n * k, max(1, n // 8) + 1):
                want = R.column(ws, lod, cx % n, cz % n, sw)
                assert R.column(big, lod, cx, cz, sb) == want, (lod, cx, cz)
                assert R.column(tiled, lod, cx, cz, st) == want, (lod, cx, cz)


def test_new_symbols_are_exported_and_wrappers_check_arguments():
    gpu_syms = open(gpu.lib_path(), "rb").read()
    assert b"cvx_set_world_repeat" in gpu_syms and "cvx_set_world_repeat" in gpu.EXPORTS
    L = host.lib()
    for name in ("cvxh_setup_lods_ex", "cvxh_render_manager_set_world_repeat"):
        assert hasattr(L, name)
    pose = host.camera_pose((1.0, 2.0, 3.0), (0.0, 0.0, 0.0), 64, 48)
    out = (C.c_float * host.LOD_LEVELS)()
    far = C.c_float()
    assert L.cvxh_setup_lods_ex(C.byref(pose), 64, 64, 48, 1.0, 2, out, C.byref(far)) != 0
    assert L.cvxh_setup_lods_ex(C.byref(pose), 64, 64, 48, 1.0, -1, out, C.byref(far)) != 0
    assert L.cvxh_render_manager_set_world_repeat(None, 1) != 0
    with pytest.raises(ValueError):
        host.setup_lods(pose, 64, 64, 48, 1.0, repeat=2)
    with pytest.raises(ValueError):
        gpu.Context.set_world_repeat(object.__new__(gpu.Context), 3)
