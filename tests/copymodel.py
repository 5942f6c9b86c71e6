"""An independent dense model of cvx_world_copy (include/cpuvox_gpu.h), written from the contract alone.

apply_copies(solid, colour, placements) -> (solid, colour): new arrays, the inputs (W, the snapshot) untouched.
  1. R = W; every placement with move = 1 turns its source box into air in R.
  2. The placements in order: the source box of W is transformed (mirror X, k quarter turns, flip Y, in that order), placed at dst, clipped to
     the volume, and the op decides each destination voxel from the source voxel s:
     REPLACE R = s (air included); FILL s solid -> R = s; CARVE s solid -> air; PAINT s solid and R solid -> s's colour.
Air voxels have colour 0 in the result."""
from __future__ import annotations

import numpy as np

FILL, CARVE, PAINT, REPLACE = 0, 1, 2, 3


def _field(p, name):
    return [int(v) for v in p[name]]


def transformed_box(box, transform):
    """The source box (an array indexed [p, q, r]) after the placement's transform, indexed by destination-local (p, q, r)."""
    if transform & 4:                                   # mirror X: p <- sx-1-p
        box = box[::-1, :, :]
    for _ in range(transform & 3):                      # (p, r, sx, sz) <- (sz-1-r, p, sz, sx)
        box = np.transpose(box, (2, 1, 0))[::-1, :, :]  # new[sz-1-r, q, p] = old[p, q, r]
    if transform & 8:                                   # flip Y: q <- sy-1-q
        box = box[:, ::-1, :]
    return box


def apply_copies(solid, colour, placements):
    dims = solid.shape
    w_solid, w_colour = solid, colour
    r_solid, r_colour = solid.copy(), colour.copy()
    for p in placements:
        if int(p["move"]):
            a, b = _field(p, "srcMin"), _field(p, "srcMax")
            r_solid[a[0]:b[0], a[1]:b[1], a[2]:b[2]] = False
    for p in placements:
        a, b, d = _field(p, "srcMin"), _field(p, "srcMax"), _field(p, "dst")
        t, op = int(p["transform"]), int(p["op"])
        s_solid = transformed_box(w_solid[a[0]:b[0], a[1]:b[1], a[2]:b[2]], t)
        s_colour = transformed_box(w_colour[a[0]:b[0], a[1]:b[1], a[2]:b[2]], t)
        # clip the destination box to the volume
        lo = [max(d[i], 0) for i in range(3)]
        hi = [min(d[i] + s_solid.shape[i], dims[i]) for i in range(3)]
        if any(lo[i] >= hi[i] for i in range(3)):
            continue
        src = tuple(slice(lo[i] - d[i], hi[i] - d[i]) for i in range(3))
        dst = tuple(slice(lo[i], hi[i]) for i in range(3))
        ss, sc = s_solid[src], s_colour[src]
        rs, rc = r_solid[dst], r_colour[dst]  # views
        if op == REPLACE:
            rs[...] = ss
            rc[...] = np.where(ss, sc, 0)
        elif op == FILL:
            rs[ss] = True
            rc[ss] = sc[ss]
        elif op == CARVE:
            rs[ss] = False
        elif op == PAINT:
            m = ss & rs
            rc[m] = sc[m]
        else:
            raise ValueError(f"bad op {op}")
    r_colour[~r_solid] = 0
    return r_solid, r_colour
