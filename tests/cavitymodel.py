"""An independent dense model of cvx_world_cavities (include/cpuvox_gpu.h), written from the contract alone: scipy.ndimage.label with the
6-neighbour structure over the AIR voxels of the clipped box, the open bits voxel by voxel on the world padded with air, then seeds, boxes,
counts and the ordered list in numpy.  It knows nothing about runs.

analyse(solid, box_min, box_max, open_faces, max_voxels) -> (cavities PIECE_DTYPE array of ALL selected cavities in the contract's order, summary
dict, mask of the selected cavities' voxels); fill(solid, colour, ..., argb) -> the world with them solid."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

from piecesmodel import PIECE_DTYPE, SIX, clip_box, rectangle  # noqa: F401  (rectangle: cvx_world_cavities' FILL rectangle is cvx_world_pieces')

OPEN_DEFAULT = 0x3B
SUMMARY_NAMES = ("enclosedCavities", "enclosedVoxels", "selectedCavities", "selectedVoxels", "openRegions", "openVoxels")


def analyse(solid, box_min, box_max, open_faces=OPEN_DEFAULT, max_voxels=0):
    dims = solid.shape
    lo, hi = clip_box(dims, box_min, box_max)
    box = tuple(slice(lo[a], hi[a]) for a in range(3))
    air = ~solid[box]
    labels, count = ndimage.label(air, structure=SIX)
    mask = np.zeros(dims, dtype=bool)
    summary = dict.fromkeys(SUMMARY_NAMES, 0)
    if count == 0:
        return np.zeros(0, dtype=PIECE_DTYPE), summary, mask
    x, y, z = np.nonzero(air)
    lab = labels[x, y, z] - 1
    g = [x + lo[0], y + lo[1], z + lo[2]]
    voxels = np.bincount(lab, minlength=count).astype(np.int64)
    # the world padded with air: what lies across a face of the box
    padded = np.zeros([d + 2 for d in dims], dtype=bool)
    padded[1:-1, 1:-1, 1:-1] = solid
    is_open = np.zeros(count, dtype=bool)
    for face in range(6):
        if not (open_faces >> face) & 1:
            continue
        a, up = face // 2, face % 2
        on_face = g[a] == (hi[a] - 1 if up else lo[a])
        across = [c[on_face] + 1 for c in g]
        across[a] = across[a] + (1 if up else -1)
        is_open[lab[on_face][~padded[across[0], across[1], across[2]]]] = True
    # the seed: first column in (x, z) order, there the highest y -> the smallest key
    key = (g[0].astype(np.int64) * dims[2] + g[2]) * dims[1] + (dims[1] - 1 - g[1])
    seed_key = np.full(count, np.iinfo(np.int64).max)
    np.minimum.at(seed_key, lab, key)
    mins = np.full((count, 3), np.iinfo(np.int64).max)
    maxs = np.full((count, 3), -1)
    for a in range(3):
        np.minimum.at(mins[:, a], lab, g[a])
        np.maximum.at(maxs[:, a], lab, g[a] + 1)
    enclosed = ~is_open
    selected = enclosed & ((voxels <= max_voxels) if max_voxels else True)
    order = [k for k in np.argsort(seed_key, kind="stable") if selected[k]]
    out = np.zeros(len(order), dtype=PIECE_DTYPE)
    dy, dz = dims[1], dims[2]
    for i, k in enumerate(order):
        out[i]["min"], out[i]["max"], out[i]["voxels"] = mins[k], maxs[k], voxels[k]
        s = int(seed_key[k])
        out[i]["seed"] = (s // (dy * dz), dy - 1 - s % dy, (s // dy) % dz)
    summary = {"enclosedCavities": int(enclosed.sum()), "enclosedVoxels": int(voxels[enclosed].sum()),
               "selectedCavities": int(selected.sum()), "selectedVoxels": int(voxels[selected].sum()),
               "openRegions": int(is_open.sum()), "openVoxels": int(voxels[is_open].sum())}
    chosen = selected[lab]
    mask[g[0][chosen], g[1][chosen], g[2][chosen]] = True
    return out, summary, mask


def fill(solid, colour, box_min, box_max, open_faces=OPEN_DEFAULT, max_voxels=0, argb=0):
    """(solid, colour) with the selected cavities solid in `argb`."""
    _, _, mask = analyse(solid, box_min, box_max, open_faces, max_voxels)
    c = colour.copy()
    c[mask] = np.uint32(argb & 0xFFFFFFFF)
    return solid | mask, c
