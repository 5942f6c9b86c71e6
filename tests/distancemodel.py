"""An independent dense model of cvx_world_distance (include/cpuvox_gpu.h), written from the contract alone.  It knows nothing about runs or
columns: the world is an (x, y, z) bool volume `solid`, as in the other models, and everything outside it follows the outside rule.

A box is (box_min, box_max) in (x, y, z); every field has shape (X, Z, Y) -- x, then z, y fastest -- and dtype int32.
  outside_solid(dims, x, y, z, solid_outside)      Solid(v) for voxels outside the world (arrays or scalars)
  volume(solid, lo, hi, solid_outside)             Solid(v) over [lo, hi), any box of space, as an (x, y, z) bool array
  field(solid, box, R, mode, solid_outside)        pads the box by R on all six sides and takes a windowed min-plus along each axis with
                                                   shifted arrays
  sparse_field(points, box, R)                     brute force over an explicit list of solid voxels: D_S of a world that holds only them and
                                                   has nothing solid outside
  brute_field(solid, box, R, mode, solid_outside)  a plain loop over every voxel of the box and every voxel of the cube of radius R around it;
                                                   for boxes of at most about 6^3 voxels"""
from __future__ import annotations

import numpy as np

FAR = 0x7FFFFFFF
TO_SOLID, TO_AIR, SIGNED = 0, 1, 2


def outside_solid(dims, x, y, z, solid_outside):
    """For voxels outside the world: solid iff on some axis the voxel lies beyond the world on the side of a face whose bit is set (faces
    0..5 = -X, +X, -Y, +Y, -Z, +Z)."""
    bit = [bool(solid_outside >> f & 1) for f in range(6)]
    out = np.zeros(np.broadcast(x, y, z).shape, dtype=bool)
    for axis, v in enumerate((x, y, z)):
        if bit[2 * axis]:
            out = out | (v < 0)
        if bit[2 * axis + 1]:
            out = out | (v >= dims[axis])
    return out


def volume(solid, lo, hi, solid_outside):
    dims = solid.shape
    x, y, z = np.meshgrid(*[np.arange(int(lo[a]), int(hi[a]), dtype=np.int64) for a in range(3)], indexing="ij", sparse=True)
    inside = (x >= 0) & (x < dims[0]) & (y >= 0) & (y < dims[1]) & (z >= 0) & (z < dims[2])
    out = outside_solid(dims, x, y, z, solid_outside) & ~inside
    a = [max(int(lo[i]), 0) for i in range(3)]
    b = [min(int(hi[i]), dims[i]) for i in range(3)]
    if all(a[i] < b[i] for i in range(3)):
        out[tuple(slice(a[i] - int(lo[i]), b[i] - int(lo[i])) for i in range(3))] = solid[tuple(slice(a[i], b[i]) for i in range(3))]
    return out


def _transform(target, R):
    """min over s with target[s] of |s - v|^2, windows of R per axis, over the whole padded array; a large value where there is none."""
    big = np.int32(1 << 28)
    f = np.where(target, np.int32(0), big)
    for axis in range(3):
        g = f.copy()
        n = f.shape[axis]
        for d in range(1, min(R, n - 1) + 1):
            near, far_ = [slice(None)] * 3, [slice(None)] * 3
            near[axis], far_[axis] = slice(d, None), slice(None, n - d)
            near, far_ = tuple(near), tuple(far_)
            np.minimum(g[near], f[far_] + np.int32(d * d), out=g[near])
            np.minimum(g[far_], f[near] + np.int32(d * d), out=g[far_])
        f = g
    return f


def _finish(values, R):
    return np.where(values <= R * R, values, FAR).astype(np.int32)


def field(solid, box, R, mode=TO_SOLID, solid_outside=0x04):
    lo, hi = [int(v) for v in box[0]], [int(v) for v in box[1]]
    s = volume(solid, [v - R for v in lo], [v + R for v in hi], solid_outside)
    crop = (slice(R, -R),) * 3
    if mode == TO_SOLID:
        out = _finish(_transform(s, R)[crop], R)
    elif mode == TO_AIR:
        out = _finish(_transform(~s, R)[crop], R)
    elif mode == SIGNED:
        out = np.where(s[crop], -_finish(_transform(~s, R)[crop], R), _finish(_transform(s, R)[crop], R)).astype(np.int32)
    else:
        raise ValueError(f"bad mode {mode}")
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def sparse_field(points, box, R):
    lo, hi = [int(v) for v in box[0]], [int(v) for v in box[1]]
    x, y, z = np.meshgrid(*[np.arange(lo[a], hi[a], dtype=np.int64) for a in range(3)], indexing="ij", sparse=True)
    best = np.full((hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]), 1 << 40, dtype=np.int64)
    for px, py, pz in points:
        np.minimum(best, (x - int(px)) ** 2 + (y - int(py)) ** 2 + (z - int(pz)) ** 2, out=best)
    return np.ascontiguousarray(_finish(best, R).transpose(0, 2, 1))


def _solid_at(solid, x, y, z, solid_outside):
    dims = solid.shape
    if 0 <= x < dims[0] and 0 <= y < dims[1] and 0 <= z < dims[2]:
        return bool(solid[x, y, z])
    v = (x, y, z)
    return any((v[a] < 0 and solid_outside >> 2 * a & 1) or (v[a] >= dims[a] and solid_outside >> (2 * a + 1) & 1) for a in range(3))


def brute_field(solid, box, R, mode=TO_SOLID, solid_outside=0x04):
    lo, hi = [int(v) for v in box[0]], [int(v) for v in box[1]]
    out = np.zeros((hi[0] - lo[0], hi[2] - lo[2], hi[1] - lo[1]), dtype=np.int32)
    for x in range(lo[0], hi[0]):
        for z in range(lo[2], hi[2]):
            for y in range(lo[1], hi[1]):
                best = {True: FAR, False: FAR}  # to the nearest solid / air voxel
                for dx in range(-R, R + 1):
                    for dy in range(-R, R + 1):
                        for dz in range(-R, R + 1):
                            dd = dx * dx + dy * dy + dz * dz
                            if dd <= R * R:
                                kind = _solid_at(solid, x + dx, y + dy, z + dz, solid_outside)
                                best[kind] = min(best[kind], dd)
                if mode == SIGNED:
                    value = -best[False] if _solid_at(solid, x, y, z, solid_outside) else best[True]
                else:
                    value = best[mode == TO_SOLID]
                out[x - lo[0], z - lo[2], y - lo[1]] = value
    return out
