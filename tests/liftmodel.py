"""An independent dense model of cvx_world_lift_pieces (include/cpuvox_gpu_lift.h), written from the header alone on top of
piecesmodel.analyse (which pieces float, in which order) and scipy.ndimage.label (which voxels belong to which piece).

lift(solid, colour, box_min, box_max, anchors, piece_capacity, voxel_capacity) -> a Lift: the listed pieces as a LIFTED_PIECE_DTYPE array
(offsets by the prefix rule, sums as Python integers modulo 2^64), the summary, the two pools as far as they are written, every stored piece's
arrays of shape (X, Z, Y), and the world after a REMOVE of the stored pieces.  mass(piece) -> centre and inertia as exact rationals."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction

import numpy as np
from scipy import ndimage

import piecesmodel

COPY, REMOVE = 0, 1
LIFTED_PIECE_DTYPE = np.dtype([("piece", piecesmodel.PIECE_DTYPE), ("offset", "<i8"), ("sum", "<u8", 3), ("moment", "<u8", 6)])
MOD = 1 << 64


@dataclass
class Lift:
    pieces: np.ndarray   # the listed pieces
    summary: dict        # cvx_pieces_summary's four, storedPieces, storedVoxels, neededVoxels
    argb: np.ndarray     # uint32, storedVoxels elements
    solid: np.ndarray    # uint8, storedVoxels elements
    models: list         # per stored piece: (argb, solid) of shape (X, Z, Y)
    removed: tuple       # (solid, colour) of the world without the stored pieces


def volume(piece) -> int:
    return int(np.prod([int(piece["max"][a]) - int(piece["min"][a]) for a in range(3)]))


def sums_of(p) -> tuple:
    """p: (n, 3) integer coordinates relative to the piece's min -> (sum[3], moment[6]) as Python integers modulo 2^64."""
    p = np.asarray(p, dtype=np.int64)
    if len(p) * max(int(p.max(initial=1)), 1) ** 2 < 1 << 62:  # no int64 sum can overflow: numpy's are the exact integers too
        s = [int(p[:, a].sum()) for a in range(3)]
        m = [int((p[:, a] * p[:, a]).sum()) for a in range(3)] + [int((p[:, i] * p[:, j]).sum()) for i, j in ((0, 1), (1, 2), (2, 0))]
        return s, m
    cols = [[int(v) for v in p[:, a]] for a in range(3)]
    s = [sum(c) % MOD for c in cols]
    m = [sum(v * v for v in c) % MOD for c in cols]
    m += [sum(a * b for a, b in zip(cols[i], cols[j])) % MOD for i, j in ((0, 1), (1, 2), (2, 0))]
    return s, m


def lift(solid, colour, box_min, box_max, anchors, piece_capacity, voxel_capacity) -> Lift:
    floating, summary, _ = piecesmodel.analyse(solid, box_min, box_max, anchors)
    lo, hi = piecesmodel.clip_box(solid.shape, box_min, box_max)
    box = tuple(slice(lo[a], hi[a]) for a in range(3))
    labels = np.zeros(solid.shape, dtype=np.int64)
    labels[box], _ = ndimage.label(solid[box], structure=piecesmodel.SIX)
    listed = floating[:max(int(piece_capacity), 0)]
    out = np.zeros(len(listed), dtype=LIFTED_PIECE_DTYPE)
    out["piece"] = listed
    used, open_, models, argb, mask = 0, True, [], [], []
    gone = np.zeros(solid.shape, dtype=bool)
    for i, piece in enumerate(listed):
        cut = tuple(slice(int(piece["min"][a]), int(piece["max"][a])) for a in range(3))
        mine = labels[cut] == labels[tuple(int(v) for v in piece["seed"])]    # (every voxel of the piece lies in its box)
        assert int(mine.sum()) == int(piece["voxels"])
        out[i]["sum"], out[i]["moment"] = sums_of(np.argwhere(mine))
        v = volume(piece)
        open_ = open_ and used + v <= voxel_capacity
        out[i]["offset"] = used if open_ else -1
        if not open_:
            continue
        used += v
        own = mine.transpose(0, 2, 1)                                        # (X, Y, Z) -> (X, Z, Y): y fastest
        words = np.where(own, colour[cut].transpose(0, 2, 1), 0).astype(np.uint32)
        models.append((words, own.astype(np.uint8)))
        argb.append(words.ravel())
        mask.append(own.astype(np.uint8).ravel())
        gone[cut] |= mine
    summary = dict(summary, storedPieces=len(models), storedVoxels=used, neededVoxels=sum(volume(p) for p in floating))
    after = solid & ~gone
    return Lift(out, summary, np.concatenate(argb) if argb else np.zeros(0, np.uint32), np.concatenate(mask) if mask else np.zeros(0, np.uint8), models,
                (after, np.where(after, colour, 0).astype(colour.dtype)))


def mass(piece):
    """A LIFTED_PIECE_DTYPE element whose sums did not wrap -> (centre[3], inertia[6] = Ixx, Iyy, Izz, Ixy, Iyz, Izx) as Fractions: unit cubes of
    unit mass, voxel v the cube [v, v + 1); about the centre of mass; each cube's own 1/6 + 1/6 = 1/3 in every diagonal term, as the header
    states it; products negative."""
    n = int(piece["piece"]["voxels"])
    s = [int(v) for v in piece["sum"]]
    m = [int(v) for v in piece["moment"]]
    c = [Fraction(s[a], n) for a in range(3)]
    centre = [int(piece["piece"]["min"][a]) + c[a] + Fraction(1, 2) for a in range(3)]
    q = [m[a] - n * c[a] * c[a] for a in range(3)]  # sum (p_a - c_a)^2
    own = Fraction(n, 3)
    diagonal = [q[1] + q[2] + own, q[2] + q[0] + own, q[0] + q[1] + own]
    products = [-(m[3 + k] - n * c[k] * c[(k + 1) % 3]) for k in range(3)]
    return centre, diagonal + products
