"""An independent model of cvx_world_read_heights / cvx_world_write_heights (include/cpuvox_gpu_heights.h), written from the contract alone, in numpy.
It knows nothing about runs or spans: a write is EXPANDED into the dense (X, Z, Y) arrays the contract defines it by and handed to
tests/densemodel.py; a read is an argmax over the model volume.  The world is a pair of (x, y, z) volumes as in the other models.

A box is (box_min, box_max) in (x, y, z); the height arrays have shape (X, Z) and may stick out of the world.
  spans(box, heights, thickness, flags) -> (b, H): per column the set voxels b <= y < H.
  expand(box, heights, argb, side, thickness, flags) -> (argb3, mask3) of shape (X, Z, Y).
  write(solid, colour, box, heights, argb, side, thickness, flags, op) -> (solid, colour) = densemodel.write of the expansion.
  read(solid, colour, box) -> (heights, argb, bottoms)."""
from __future__ import annotations

import numpy as np

import densemodel

WALLED = 1


def spans(box, heights, thickness, flags):
    y0, y1 = int(box[0][1]), int(box[1][1])
    H = np.clip(np.asarray(heights, dtype=np.int64), y0, y1)
    assert H.shape == (int(box[1][0]) - int(box[0][0]), int(box[1][2]) - int(box[0][2])), H.shape
    if thickness == 0:
        return np.full(H.shape, y0, dtype=np.int64), H
    pad = np.pad(H, 1, mode="constant", constant_values=y0) if flags & WALLED else np.pad(H, 1, mode="edge")
    N = np.minimum(np.minimum(pad[:-2, 1:-1], pad[2:, 1:-1]), np.minimum(pad[1:-1, :-2], pad[1:-1, 2:]))
    return np.maximum(y0, np.minimum(H, N) - thickness), H


def expand(box, heights, argb, side, thickness, flags):
    y0, y1 = int(box[0][1]), int(box[1][1])
    b, H = spans(box, heights, thickness, flags)
    y = np.arange(y0, y1, dtype=np.int64)[None, None, :]
    mask = (b[:, :, None] <= y) & (y < H[:, :, None])
    if argb is None:
        return None, mask
    top = np.asarray(argb, dtype=np.uint32)[:, :, None]
    below = top if side is None else np.asarray(side, dtype=np.uint32)[:, :, None]
    colours = np.where(y == H[:, :, None] - 1, top, below)
    return np.where(mask, colours, 0).astype(np.uint32), mask


def write(solid, colour, box, heights, argb, side, thickness, flags, op):
    argb3, mask3 = expand(box, heights, argb, side, thickness, flags)
    return densemodel.write(solid, colour, box, argb3, mask3, op)


def read(solid, colour, box):
    (x0, y0, z0), (x1, y1, z1) = [[int(v) for v in c] for c in box]
    heights = np.full((x1 - x0, z1 - z0), y0, dtype=np.int32)
    argb = np.zeros(heights.shape, dtype=np.uint32)
    bottoms = heights.copy()
    lo, hi = max(y0, 0), min(y1, solid.shape[1])
    for bx in range(x1 - x0):
        for bz in range(z1 - z0):
            x, z = x0 + bx, z0 + bz
            if not (0 <= x < solid.shape[0] and 0 <= z < solid.shape[2]) or lo >= hi:
                continue
            ys = np.nonzero(solid[x, lo:hi, z])[0]
            if len(ys) == 0:
                continue
            top = lo + int(ys[-1])
            air = np.nonzero(~solid[x, lo:top, z])[0]
            heights[bx, bz] = top + 1
            argb[bx, bz] = colour[x, top, z]
            bottoms[bx, bz] = lo + int(air[-1]) + 1 if len(air) else lo
    return heights, argb, bottoms
