"""An independent dense model of cvx_world_surface_rects (include/cpuvox_gpu_surface_rects.h), written from the contract alone on top of the dense
model of cvx_world_surface (tests/surfacemodel.py).  It knows nothing about pairs, cursors or columns: the quads of surfacemodel.surface become
items (voxel, size, face, argb), a merge pass is a dictionary from (face, lowest voxel) to the item and a walk along the "follows" links, and the
list is sorted by the stated key.

rects(solid, colour, box_min, box_max, solid_outside, flags) -> (RECT_DTYPE array of ALL rectangles in the contract's order, summary dict);
unit_faces(rects) -> the (x, y, z, face) rows of the voxel faces the rectangles cover; whole_edge_pairs(rects, ignore) -> how many pairs of
rectangles of one face, one plane and one key (the colour, unless colours are ignored) share a whole edge (the rule leaves none)."""
from __future__ import annotations

import numpy as np

import surfacemodel

IGNORE_COLOUR = surfacemodel.IGNORE_COLOUR
RECT_DTYPE = np.dtype([("voxel", "<i4", 3), ("size", "<i4", 3), ("face", "<i4"), ("argb", "<u4")])
SUMMARY_NAMES = ("rects", "strips", "unitFaces", "rectsPerFace")
PASSES = ((2, {0, 1}), (0, {2, 3, 4, 5}), (2, {2, 3}))  # (axis, faces): -X / +X along z; the others along x; then the rows of -Y / +Y along z


def merge_pass(items, axis, faces, ignore):
    """One pass along `axis` over the items (tuples voxel, size, face, argb) whose face is in `faces`; the others pass through."""
    others = [a for a in range(3) if a != axis]
    at = {(face, voxel): k for k, (voxel, size, face, argb) in enumerate(items) if face in faces}
    follower, follows = {}, set()
    for k, (voxel, size, face, argb) in enumerate(items):
        if face not in faces:
            continue
        behind = list(voxel)
        behind[axis] += size[axis]
        q = at.get((face, tuple(behind)))
        if q is None:
            continue
        _, q_size, _, q_argb = items[q]
        if all(q_size[a] == size[a] for a in others) and (ignore or q_argb == argb):
            assert q not in follows
            follower[k] = q
            follows.add(q)
    out = []
    for k, (voxel, size, face, argb) in enumerate(items):
        if face not in faces:
            out.append(items[k])
            continue
        if k in follows:
            continue
        total, link = size[axis], k
        while link in follower:
            link = follower[link]
            total += items[link][1][axis]
        merged = list(size)
        merged[axis] = total
        out.append((voxel, tuple(merged), face, argb))
    return out


def rects(solid, colour, box_min, box_max, solid_outside=surfacemodel.OUTSIDE_DEFAULT, flags=0):
    quads, strips = surfacemodel.surface(solid, colour, box_min, box_max, solid_outside, flags)
    ignore = bool(flags & IGNORE_COLOUR)
    items = [(tuple(v), (1, n, 1), f, c) for v, n, f, c in zip(quads["voxel"].tolist(), quads["length"].tolist(), quads["face"].tolist(), quads["argb"].tolist())]
    for axis, faces in PASSES:
        items = merge_pass(items, axis, faces, ignore)
    items.sort(key=lambda i: (i[0][0], i[0][2], i[2], -(i[0][1] + i[1][1])))
    out = np.zeros(len(items), dtype=RECT_DTYPE)
    if items:
        out["voxel"], out["size"] = [i[0] for i in items], [i[1] for i in items]
        out["face"], out["argb"] = [i[2] for i in items], [i[3] for i in items]
    summary = {"rects": len(out), "strips": strips["quads"], "unitFaces": strips["unitFaces"],
               "rectsPerFace": [int((out["face"] == f).sum()) for f in range(6)]}
    return out, summary


def unit_faces(rects):
    """One row (x, y, z, face) per voxel face the rectangles cover."""
    size = rects["size"].astype(np.int64)
    count = size.prod(axis=1)
    base = np.repeat(np.arange(len(rects)), count)
    step = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count)
    sy, sz = size[base, 1], size[base, 2]
    out = np.zeros((len(base), 4), dtype=np.int64)
    out[:, 0] = rects["voxel"][base, 0] + step // (sy * sz)
    out[:, 1] = rects["voxel"][base, 1] + (step // sz) % sy
    out[:, 2] = rects["voxel"][base, 2] + step % sz
    out[:, 3] = rects["face"][base]
    return out


def whole_edge_pairs(rects, ignore):
    """Pairs (p, q) of one face, one plane and one key where q starts where p ends along an in-plane axis and both have the same start and the
    same size along the other one: the two would be one rectangle."""
    at = {}
    for voxel, size, face, argb in zip(rects["voxel"].tolist(), rects["size"].tolist(), rects["face"].tolist(), rects["argb"].tolist()):
        key = (face, 0 if ignore else argb, tuple(voxel))
        assert key not in at
        at[key] = tuple(size)
    pairs = 0
    for (face, colour, voxel), size in at.items():
        in_plane = [a for a in range(3) if a != face // 2]
        for a, b in (in_plane, in_plane[::-1]):
            behind = list(voxel)
            behind[a] += size[a]
            other = at.get((face, colour, tuple(behind)))
            pairs += other is not None and other[b] == size[b]
    return pairs
