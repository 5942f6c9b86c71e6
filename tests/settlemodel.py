"""An independent dense model of cvx_world_settle (include/cpuvox_gpu.h), written from the contract's STEP rule alone: the floating pieces are
piecesmodel.analyse's; then, one voxel at a time, the largest set M of pieces with nothing static and no piece outside M directly under any of
their voxels is found by removing blocked pieces to a fixpoint on the label volume, and M moves down by one, until M is empty or max_drop steps
have been made.

settle(solid, colour, box_min, box_max, anchors, max_drop) -> (pieces PIECE_DTYPE array of ALL floating pieces before the fall in the contract's
order, their drops as an int32 array, summary dict, (solid, colour) after the fall)."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

import piecesmodel


def settle(solid, colour, box_min, box_max, anchors, max_drop=0):
    pieces, found, mask = piecesmodel.analyse(solid, box_min, box_max, anchors)
    m = len(pieces)
    summary = {"floatingPieces": found["floatingPieces"], "floatingVoxels": found["floatingVoxels"], "fallenPieces": 0, "fallenVoxels": 0, "largestDrop": 0}
    drops = np.zeros(m, dtype=np.int32)
    if m == 0:
        return pieces, drops, summary, (solid.copy(), np.where(solid, colour, 0).astype(colour.dtype))
    # the label volume: 0 = no floating voxel, i + 1 = a voxel of pieces[i] (two floating pieces never share a face, so labelling the mask separates them)
    found_labels, count = ndimage.label(mask, structure=piecesmodel.SIX)
    assert count == m
    to_place = np.zeros(count + 1, dtype=np.int64)
    for i, p in enumerate(pieces):
        to_place[found_labels[tuple(p["seed"])]] = i + 1
    assert (to_place[1:] > 0).all()
    static = solid & ~mask
    gx, gy, gz = np.nonzero(mask)
    piece = to_place[found_labels[gx, gy, gz]] - 1
    # only voxels with no voxel of their own piece directly beneath can be blocked (pieces are rigid: that stays so)
    own_below = np.zeros(len(gx), dtype=bool)
    inner = gy > 0
    own_below[inner] = mask[gx[inner], gy[inner] - 1, gz[inner]]
    bx, by, bz, bp = gx[~own_below], gy[~own_below], gz[~own_below], piece[~own_below]
    steps = 0
    while max_drop == 0 or steps < max_drop:
        labels = np.zeros(solid.shape, dtype=np.int64)
        labels[gx, gy - drops[piece], gz] = piece + 1
        y = by - drops[bp]
        under = np.maximum(y - 1, 0)
        blocked_voxel = (y == 0) | static[bx, under, bz]
        rests_on = np.where(blocked_voxel, 0, labels[bx, under, bz])  # the piece (+ 1) directly under the voxel, 0: air (or blocked anyway)
        moving = np.ones(m, dtype=bool)
        moving[bp[blocked_voxel]] = False
        while True:  # a piece over a piece that does not move does not move
            held = (rests_on > 0) & ~moving[np.maximum(rests_on - 1, 0)]
            stuck = np.zeros(m, dtype=bool)
            stuck[bp[held]] = True
            if not (stuck & moving).any():
                break
            moving &= ~stuck
        if not moving.any():
            break
        drops[moving] += 1
        steps += 1
    new_solid = static.copy()
    new_colour = np.where(static, colour, 0).astype(colour.dtype)
    new_solid[gx, gy - drops[piece], gz] = True
    new_colour[gx, gy - drops[piece], gz] = colour[gx, gy, gz]
    assert int(new_solid.sum()) == int(solid.sum()), "two voxels ended in one place"
    fell = drops > 0
    summary["fallenPieces"] = int(fell.sum())
    summary["fallenVoxels"] = int(pieces["voxels"][fell].sum())
    summary["largestDrop"] = int(drops.max())
    return pieces, drops, summary, (new_solid, new_colour)
