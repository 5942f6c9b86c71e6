"""An independent numpy model of cvx_world_place_models / cvx_world_read_model / cvx_model_instance_from_matrix (include/cpuvox_gpu_models.h),
written from the contract alone.  It knows nothing about runs: the world is a pair of (x, y, z) volumes, `solid` (bool) and `colour` (uint32,
0 for air), as in the other models.

A map is (m, t): a 3 x 3 and a 3-vector of Python / int64 integers in units of 2^-16.  A model is (argb, mask), arrays of shape (X, Z, Y) or
None.  An instance is a dict(m, t, box_min, box_max, model, op).
  apply_map(m, t, v)             -> the image of the voxels v (..., 3), int64
  place(solid, colour, models, instances) -> (solid, colour): new arrays, the contract applied voxel by voxel, instance after instance
  read(solid, colour, size, m, t)  -> (argb, mask) of shape (sx, sz, sy)
  instance_from_matrix(forward, size) -> (m, t, box_min, box_max), the helper's formula in float64
  rectangle(instances, dims, level_count) -> the call's rectangle or None"""
from __future__ import annotations

import numpy as np

FILL, CARVE, PAINT, REPLACE = 0, 1, 2, 3


def apply_map(m, t, v):
    v = np.asarray(v, dtype=np.int64)
    m = np.asarray(m, dtype=np.int64)
    t = np.asarray(t, dtype=np.int64)
    q = (m[:, 0] * (2 * v[..., 0:1] + 1) + m[:, 1] * (2 * v[..., 1:2] + 1) + m[:, 2] * (2 * v[..., 2:3] + 1)) + 2 * t
    return q >> 17  # (numpy's shift of a signed integer is arithmetic: floor)


def from_struct(instance):
    """A gpu.ModelInstance as the model's dict."""
    return dict(m=[[int(instance.toModel.m[i][j]) for j in range(3)] for i in range(3)], t=[int(v) for v in instance.toModel.t],
                box_min=[int(v) for v in instance.boxMin], box_max=[int(v) for v in instance.boxMax], model=int(instance.model), op=int(instance.op))


def _clipped(instance, dims):
    lo = [max(int(instance["box_min"][i]), 0) for i in range(3)]
    hi = [min(int(instance["box_max"][i]), dims[i]) for i in range(3)]
    return (lo, hi) if all(lo[i] < hi[i] for i in range(3)) else None


def place(solid, colour, models, instances):
    s, c = solid.copy(), colour.copy()
    for inst in instances:
        clip = _clipped(inst, solid.shape)
        if clip is None:
            continue
        lo, hi = clip
        argb, mask = models[inst["model"]]
        shape = (argb if argb is not None else mask).shape  # (X, Z, Y)
        size = (shape[0], shape[2], shape[1])
        d = np.stack(np.meshgrid(*[np.arange(lo[i], hi[i], dtype=np.int64) for i in range(3)], indexing="ij"), axis=-1)
        src = apply_map(inst["m"], inst["t"], d)
        inside = np.ones(d.shape[:-1], dtype=bool)
        for i in range(3):
            inside &= (src[..., i] >= 0) & (src[..., i] < size[i])
        sx, sy, sz = [np.where(inside, src[..., i], 0) for i in range(3)]
        a = np.asarray(argb, dtype=np.uint32)[sx, sz, sy] if argb is not None else np.zeros(inside.shape, dtype=np.uint32)
        is_set = (np.asarray(mask)[sx, sz, sy] != 0) if mask is not None else (a != 0)
        world = tuple(slice(lo[i], hi[i]) for i in range(3))
        ws, wc = s[world], c[world]  # views
        op = inst["op"]
        if op == REPLACE:
            ws[inside] = is_set[inside]
            wc[inside] = np.where(is_set, a, 0)[inside]
        elif op == FILL:
            k = inside & is_set
            ws[k] = True
            wc[k] = a[k]
        elif op == CARVE:
            if argb is None and mask is None:
                raise ValueError("a model with neither array")
            ws[inside & is_set] = False
        elif op == PAINT:
            k = inside & is_set & ws
            wc[k] = a[k]
        else:
            raise ValueError(f"bad op {op}")
        c[~s] = 0
    return s, c


def read(solid, colour, size, m, t):
    sx, sy, sz = [int(v) for v in size]
    v = np.stack(np.meshgrid(np.arange(sx, dtype=np.int64), np.arange(sy, dtype=np.int64), np.arange(sz, dtype=np.int64), indexing="ij"), axis=-1)
    d = apply_map(m, t, v)
    inside = np.ones(d.shape[:-1], dtype=bool)
    for i in range(3):
        inside &= (d[..., i] >= 0) & (d[..., i] < solid.shape[i])
    x, y, z = [np.where(inside, d[..., i], 0) for i in range(3)]
    mask = inside & solid[x, y, z]
    argb = np.where(mask, colour[x, y, z], 0).astype(np.uint32)
    return np.ascontiguousarray(argb.transpose(0, 2, 1)), np.ascontiguousarray(mask.transpose(0, 2, 1))  # (X, Y, Z) -> (X, Z, Y)


def instance_from_matrix(forward, size):
    """The helper's formula: inverse by adjugate / determinant, m = round(inv * 65536), t = round(-inv b * 65536), the box floor / ceil of the eight
    mapped corners widened by one voxel and clamped to +-2^30.  On exactly representable inputs every step is exact, whatever the order."""
    f = np.asarray(forward, dtype=np.float64).reshape(3, 4)
    a, b = f[:, :3], f[:, 3]
    det = a[0, 0] * (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) + a[0, 1] * (a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]) + a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0])
    adj = np.array([[a[(j + 1) % 3, (i + 1) % 3] * a[(j + 2) % 3, (i + 2) % 3] - a[(j + 1) % 3, (i + 2) % 3] * a[(j + 2) % 3, (i + 1) % 3] for j in range(3)]
                    for i in range(3)])
    inv = adj / det
    half_away = lambda v: int(np.sign(v) * np.floor(abs(v) + 0.5))  # noqa: E731  (llround: halves away from zero)
    m = [[half_away(inv[i, j] * 65536.0) for j in range(3)] for i in range(3)]
    t = [half_away(-(inv[i] @ b) * 65536.0) for i in range(3)]
    corners = np.array([[x, y, z] for x in (0, size[0]) for y in (0, size[1]) for z in (0, size[2])], dtype=np.float64) @ a.T + b
    lo = np.maximum(np.floor(corners.min(axis=0)) - 1, -(1 << 30)).astype(np.int64)
    hi = np.minimum(np.ceil(corners.max(axis=0)) + 1, 1 << 30).astype(np.int64)
    return m, t, lo.tolist(), hi.tolist()


def rectangle(instances, dims, level_count):
    """(x0, z0, sizeX, sizeZ): the XZ bounding box of the instances' boxes clipped to the world, rounded outward to multiples of 2^level_count
    and clipped again; None when every box lies outside the world."""
    clips = [c for c in (_clipped(i, dims) for i in instances) if c is not None]
    if not clips:
        return None
    x0, z0 = min(c[0][0] for c in clips), min(c[0][2] for c in clips)
    x1, z1 = max(c[1][0] for c in clips), max(c[1][2] for c in clips)
    k = (1 << level_count) - 1
    x0, z0 = x0 & ~k, z0 & ~k
    x1, z1 = min((x1 + k) & ~k, dims[0]), min((z1 + k) & ~k, dims[2])
    return x0, z0, x1 - x0, z1 - z0
