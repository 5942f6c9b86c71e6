"""An independent dense model of cvx_world_pieces (include/cpuvox_gpu.h), written from the contract alone: scipy.ndimage.label with the
6-neighbour structure over the dense boolean volume, then seeds, boxes, counts, anchor bits and the ordered floating list in numpy.

analyse(solid, box_min, box_max, anchors) -> (pieces PIECE_DTYPE array of ALL floating pieces in the contract's order, summary dict, mask of the
floating voxels); remove(solid, colour, ...) -> the world without them."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

GROUND, OUTSIDE, LARGEST = 1, 2, 4
PIECE_DTYPE = np.dtype([("min", "<i4", 3), ("max", "<i4", 3), ("seed", "<i4", 3), ("pad_", "<i4"), ("voxels", "<i8")])
SIX = ndimage.generate_binary_structure(3, 1)


def clip_box(dims, box_min, box_max):
    lo = [max(int(box_min[a]), 0) for a in range(3)]
    hi = [min(int(box_max[a]), dims[a]) for a in range(3)]
    return (lo, hi) if all(lo[a] < hi[a] for a in range(3)) else None


def analyse(solid, box_min, box_max, anchors):
    lo, hi = clip_box(solid.shape, box_min, box_max)
    box = tuple(slice(lo[a], hi[a]) for a in range(3))
    sub = solid[box]
    labels, count = ndimage.label(sub, structure=SIX)
    floating_mask = np.zeros(solid.shape, dtype=bool)
    summary = {"floatingPieces": 0, "floatingVoxels": 0, "anchoredPieces": 0, "anchoredVoxels": 0}
    if count == 0:
        return np.zeros(0, dtype=PIECE_DTYPE), summary, floating_mask
    x, y, z = np.nonzero(sub)
    lab = labels[x, y, z] - 1
    gx, gy, gz = x + lo[0], y + lo[1], z + lo[2]
    voxels = np.bincount(lab, minlength=count).astype(np.int64)
    # the seed: first column in (x, z) order, there the highest y -> the smallest key
    key = (gx.astype(np.int64) * solid.shape[2] + gz) * solid.shape[1] + (solid.shape[1] - 1 - gy)
    seed_key = np.full(count, np.iinfo(np.int64).max)
    np.minimum.at(seed_key, lab, key)
    mins = np.full((count, 3), np.iinfo(np.int64).max)
    maxs = np.full((count, 3), -1)
    for a, g in enumerate((gx, gy, gz)):
        np.minimum.at(mins[:, a], lab, g)
        np.maximum.at(maxs[:, a], lab, g + 1)
    anchored = np.zeros(count, dtype=bool)
    if anchors & GROUND:
        anchored[lab[gy == 0]] = True
    if anchors & OUTSIDE:
        rest = solid.copy()
        rest[box] = False  # the solid voxels of the world outside the box
        near = np.zeros(solid.shape, dtype=bool)
        for a in range(3):
            for step in (1, -1):
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[a] = slice(1, None) if step == 1 else slice(None, -1)
                dst[a] = slice(None, -1) if step == 1 else slice(1, None)
                near[tuple(dst)] |= rest[tuple(src)]
        anchored[lab[near[gx, gy, gz]]] = True
    if anchors & LARGEST:
        most = voxels.max()
        ties = np.nonzero(voxels == most)[0]
        anchored[ties[np.argmin(seed_key[ties])]] = True
    order = np.argsort(seed_key, kind="stable")
    floating = [k for k in order if not anchored[k]]
    out = np.zeros(len(floating), dtype=PIECE_DTYPE)
    dy, dz = solid.shape[1], solid.shape[2]
    for i, k in enumerate(floating):
        out[i]["min"], out[i]["max"], out[i]["voxels"] = mins[k], maxs[k], voxels[k]
        s = int(seed_key[k])
        out[i]["seed"] = (s // (dy * dz), dy - 1 - s % dy, (s // dy) % dz)
    summary = {"floatingPieces": len(floating), "floatingVoxels": int(voxels[~anchored].sum()),
               "anchoredPieces": int(anchored.sum()), "anchoredVoxels": int(voxels[anchored].sum())}
    gone = ~anchored[lab]
    floating_mask[gx[gone], gy[gone], gz[gone]] = True
    return out, summary, floating_mask


def remove(solid, colour, box_min, box_max, anchors):
    """(solid, colour) without the floating pieces; air has colour 0."""
    _, _, mask = analyse(solid, box_min, box_max, anchors)
    s = solid & ~mask
    c = np.where(s, colour, 0).astype(colour.dtype)
    return s, c


def rectangle(pieces, dims, level_count):
    """cvx_world_pieces' REMOVE rectangle (x0, z0, sizeX, sizeZ), or None when nothing floats."""
    if len(pieces) == 0:
        return None
    m = (1 << level_count) - 1
    x0, z0 = int(pieces["min"][:, 0].min()) & ~m, int(pieces["min"][:, 2].min()) & ~m
    x1, z1 = min((int(pieces["max"][:, 0].max()) + m) & ~m, dims[0]), min((int(pieces["max"][:, 2].max()) + m) & ~m, dims[2])
    return x0, z0, x1 - x0, z1 - z0


def decode_blob(blob, dims):
    """A LOD-0 world blob in the reference's layout (12-byte RLEColumn headers in x-major order, then the element pool: per column a guard, the
    runs as colorsIndex | length << 16 from the top, a guard, the colours) -> dense (solid, colour) arrays indexed [x, y, z]."""
    dx, dy, dz = dims
    raw = np.frombuffer(blob, dtype=np.uint8)
    headers = raw[:12 * dx * dz].view(np.uint32).reshape(dx * dz, 3)
    pool = raw[12 * dx * dz:].view(np.uint32) if len(raw) > 12 * dx * dz else np.zeros(0, dtype=np.uint32)
    solid = np.zeros(dims, dtype=bool)
    colour = np.zeros(dims, dtype=np.uint32)
    for i in np.nonzero(headers[:, 1] & 0xFFFF)[0]:
        off, runs = int(headers[i, 0]), int(headers[i, 1] & 0xFFFF)
        x, z = divmod(int(i), dz)
        words = pool[off + 1:off + 1 + runs]
        colours = pool[off + 2 + runs:]
        top = dy
        for w in words.tolist():
            ci, n = w & 0xFFFF, w >> 16
            if ci != 0xFFFF:
                solid[x, top - n:top, z] = True
                colour[x, top - n:top, z] = colours[ci:ci + n][::-1]
            top -= n
    return solid, colour
