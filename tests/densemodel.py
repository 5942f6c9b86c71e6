"""An independent dense model of cvx_world_read_voxels / cvx_world_write_voxels (include/cpuvox_gpu.h), written from the contract alone.  It
knows nothing about runs: the world is a pair of (x, y, z) volumes, `solid` (bool) and `colour` (uint32, 0 for air), as in the other models.

A box is (box_min, box_max) in (x, y, z); the dense arrays have shape (X, Z, Y) -- x, then z, y fastest -- and may stick out of the world.
  read(solid, colour, box) -> (argb, mask): the colour word / 1 of a solid voxel, 0 for air and outside the world.
  write(solid, colour, box, argb, mask, op) -> (solid, colour): new arrays.  A box voxel is SET iff mask != 0 when there is a mask, else iff
    argb != 0.  REPLACE: the voxel becomes solid(argb) when set, else air; FILL: set -> solid(argb); CARVE: set -> air; PAINT: set and solid
    -> takes argb.  Voxels outside the world are dropped.  Air voxels have colour 0 in the result."""
from __future__ import annotations

import numpy as np

FILL, CARVE, PAINT, REPLACE = 0, 1, 2, 3


def _clip(solid, box):
    """(slices into the world, slices into the box's (X, Y, Z) array), or None when the box misses the world."""
    lo, hi = [int(v) for v in box[0]], [int(v) for v in box[1]]
    a = [max(lo[i], 0) for i in range(3)]
    b = [min(hi[i], solid.shape[i]) for i in range(3)]
    if any(a[i] >= b[i] for i in range(3)):
        return None
    return tuple(slice(a[i], b[i]) for i in range(3)), tuple(slice(a[i] - lo[i], b[i] - lo[i]) for i in range(3))


def read(solid, colour, box):
    size = [int(box[1][i]) - int(box[0][i]) for i in range(3)]
    argb = np.zeros(size, dtype=np.uint32)  # (X, Y, Z)
    mask = np.zeros(size, dtype=bool)
    clip = _clip(solid, box)
    if clip is not None:
        world, local = clip
        mask[local] = solid[world]
        argb[local] = np.where(solid[world], colour[world], 0)
    return np.ascontiguousarray(argb.transpose(0, 2, 1)), np.ascontiguousarray(mask.transpose(0, 2, 1))


def write(solid, colour, box, argb, mask, op):
    s, c = solid.copy(), colour.copy()
    size = tuple(int(box[1][i]) - int(box[0][i]) for i in range(3))
    if argb is None:
        if op != CARVE or mask is None:
            raise ValueError("argb may be left out only for a CARVE with a mask")
        argb = np.zeros((size[0], size[2], size[1]), dtype=np.uint32)
    argb = np.asarray(argb, dtype=np.uint32).transpose(0, 2, 1)  # -> (X, Y, Z)
    is_set = (np.asarray(mask).transpose(0, 2, 1) != 0) if mask is not None else (argb != 0)
    assert argb.shape == size and is_set.shape == size, (argb.shape, is_set.shape, size)
    clip = _clip(solid, box)
    if clip is None:
        return s, c
    world, local = clip
    a, m = argb[local], is_set[local]
    ws, wc = s[world], c[world]  # views
    if op == REPLACE:
        ws[...] = m
        wc[...] = np.where(m, a, 0)
    elif op == FILL:
        ws[m] = True
        wc[m] = a[m]
    elif op == CARVE:
        ws[m] = False
    elif op == PAINT:
        k = m & ws
        wc[k] = a[k]
    else:
        raise ValueError(f"bad op {op}")
    c[~s] = 0
    return s, c


def rectangle(box, dims, level_count):
    """The call's rectangle (x0, z0, sizeX, sizeZ): the box clipped to the world, its XZ footprint rounded outward to multiples of
    2^level_count and clipped again; None when the box lies outside the world."""
    lo = [max(int(box[0][i]), 0) for i in range(3)]
    hi = [min(int(box[1][i]), dims[i]) for i in range(3)]
    if any(lo[i] >= hi[i] for i in range(3)):
        return None
    m = (1 << level_count) - 1
    x0, z0 = lo[0] & ~m, lo[2] & ~m
    x1, z1 = min((hi[0] + m) & ~m, dims[0]), min((hi[2] + m) & ~m, dims[2])
    return x0, z0, x1 - x0, z1 - z0
