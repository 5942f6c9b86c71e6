"""An independent dense model of cvx_world_surface (include/cpuvox_gpu.h), written from the contract alone.  It knows nothing about runs: the
solid array is padded with what solidOutside says lies across each face of the world, the exposed faces are shifted comparisons, the quads are
formed by scanning every column voxel by voxel from the top, and the list is sorted by the stated key.

surface(solid, colour, box_min, box_max, solid_outside, flags) -> (quads QUAD_DTYPE array of ALL quads in the contract's order, summary dict);
unit_faces(quads) -> the (x, y, z, face) rows of the exposed voxel faces the quads cover; open_edges(faces) -> how many edges of the unit squares
are shared by an odd number of them (0: the surface is closed)."""
from __future__ import annotations

import numpy as np

from piecesmodel import clip_box

OUTSIDE_DEFAULT = 0x04
IGNORE_COLOUR = 1
QUAD_DTYPE = np.dtype([("voxel", "<i4", 3), ("face", "<i4"), ("length", "<i4"), ("argb", "<u4")])
SUMMARY_NAMES = ("quads", "unitFaces", "quadsPerFace")


def exposed(solid, solid_outside=OUTSIDE_DEFAULT):
    """exposed[f][x, y, z]: voxel (x, y, z) is solid and the voxel across its face f (0..5 = -X, +X, -Y, +Y, -Z, +Z) is air."""
    padded = np.zeros([d + 2 for d in solid.shape], dtype=bool)
    for face in range(6):  # the slab across face f of the world
        slab = [slice(None)] * 3
        slab[face // 2] = -1 if face % 2 else 0
        padded[tuple(slab)] = bool((solid_outside >> face) & 1)
    padded[1:-1, 1:-1, 1:-1] = solid
    out = []
    for face in range(6):
        across = [slice(1, -1)] * 3
        across[face // 2] = slice(2, None) if face % 2 else slice(0, -2)
        out.append(solid & ~padded[tuple(across)])
    return out


def surface(solid, colour, box_min, box_max, solid_outside=OUTSIDE_DEFAULT, flags=0):
    dims = solid.shape
    lo, hi = clip_box(dims, box_min, box_max)
    inside = np.zeros(dims, dtype=bool)
    inside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    ignore = bool(flags & IGNORE_COLOUR)
    parts = []  # per face: x, z, face, top, bottom, argb of its quads
    for face, mask in enumerate(exposed(solid, solid_outside)):
        x, y, z = np.nonzero(mask & inside)
        if len(x) == 0:
            continue
        order = np.lexsort((-y, z, x))  # column after column, every column from its top voxel down
        x, y, z = x[order], y[order], z[order]
        c = colour[x, y, z]
        # voxel k continues the quad of voxel k - 1: same column, directly below it, a side face, and the same colour unless colours are ignored
        joins = np.zeros(len(x), dtype=bool)
        if face not in (2, 3):
            joins[1:] = (x[1:] == x[:-1]) & (z[1:] == z[:-1]) & (y[1:] == y[:-1] - 1) & (ignore | (c[1:] == c[:-1]))
        first = np.nonzero(~joins)[0]
        last = np.append(first[1:], len(x)) - 1
        parts.append(np.stack([x[first], z[first], np.full(len(first), face), y[first], y[last], c[first].astype(np.int64)], axis=1))
    rows = np.concatenate(parts) if parts else np.zeros((0, 6), dtype=np.int64)
    rows = rows[np.lexsort((-rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))]  # ascending x, z, face, then descending top
    quads = np.zeros(len(rows), dtype=QUAD_DTYPE)
    quads["voxel"][:, 0], quads["voxel"][:, 1], quads["voxel"][:, 2] = rows[:, 0], rows[:, 4], rows[:, 1]
    quads["face"], quads["length"], quads["argb"] = rows[:, 2], rows[:, 3] - rows[:, 4] + 1, rows[:, 5].astype(np.uint32)
    summary = {"quads": len(rows), "unitFaces": int(quads["length"].sum()), "quadsPerFace": [int((quads["face"] == f).sum()) for f in range(6)]}
    return quads, summary


def unit_faces(quads):
    """One row (x, y, z, face) per exposed voxel face the quads cover."""
    reps = quads["length"].astype(np.int64)
    base = np.repeat(np.arange(len(quads)), reps)
    step = np.arange(int(reps.sum())) - np.repeat(np.cumsum(reps) - reps, reps)
    out = np.zeros((len(base), 4), dtype=np.int64)
    out[:, 0], out[:, 2], out[:, 3] = quads["voxel"][base, 0], quads["voxel"][base, 2], quads["face"][base]
    out[:, 1] = quads["voxel"][base, 1] + step
    return out


def open_edges(faces):
    """The edges of the unit squares of `faces` (rows x, y, z, face) that an odd number of them share."""
    edges = []
    for x, y, z, face in faces.tolist():
        axis, up = face // 2, face % 2
        corner = [x, y, z]
        corner[axis] += up
        u, v = [a for a in range(3) if a != axis]
        for direction, along, offset in ((u, v, 0), (u, v, 1), (v, u, 0), (v, u, 1)):  # the edge runs along `direction`, at `offset` on the other axis
            start = list(corner)
            start[along] += offset
            edges.append((*start, direction))
    if not edges:
        return 0
    _, counts = np.unique(np.array(edges, dtype=np.int64), axis=0, return_counts=True)
    return int((counts % 2).sum())
