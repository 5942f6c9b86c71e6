"""An independent dense model of cvx_world_light_lamps (include/cpuvox_gpu.h), written from the contract alone: lightmodel.shades for the floor, sky
and sun, and for the lamps a fractions.Fraction walk per (voxel, lamp) pair with numpy for facing and the term.

lamp(pos, radius, level) -> a lamp; lamp_sum(solid, p, lamps) -> (the summed lamp terms as a volume, statistics of the pairs);
shades(solid, p, lamps) -> (mask of the lit voxels, their shade volume); light(solid, colour, p, lamps) -> the new colour volume.

The walk of D = L - v depends on D alone, and a reflection of an axis reflects it (a crossing parameter (2k - 1) / |D_i| holds only |D_i|): the
voxel sequence is computed once per (|D_x|, |D_y|, |D_z|) and signed per pair.  The pairs of a lamp are then tested together."""
from __future__ import annotations

from fractions import Fraction
from functools import lru_cache

import numpy as np

import lightmodel


def lamp(pos, radius, level):
    return dict(pos=[int(v) for v in pos], radius=int(radius), level=int(level))


def words(lamps):
    """count, then x y z radius level per lamp (tests/lamp_rules.cpp)."""
    return [len(lamps)] + [v for l in lamps for v in (*l["pos"], l["radius"], l["level"])]


def tuples(lamps):
    """What Context.world_light_lamps takes."""
    return [(l["pos"], l["radius"], l["level"]) for l in lamps]


@lru_cache(maxsize=None)
def walk(d):
    """d = (|D_x|, |D_y|, |D_z|) != 0 -> (the voxels the walk reaches BEFORE it arrives at d, relative to the start, as an (n, 3) array; whether a
    step advanced two or three axes at once: the ray passed exactly through a voxel edge or corner)."""
    k, pos, out, tie = [1, 1, 1], [0, 0, 0], [], False
    pending = {a: Fraction(1, d[a]) for a in range(3) if d[a] != 0}
    for _ in range(sum(d)):
        t = min(pending.values())
        moved = [a for a, ta in pending.items() if ta == t]
        for a in moved:
            pos[a] += 1
            k[a] += 1
            pending[a] = Fraction(2 * k[a] - 1, d[a])
        tie |= len(moved) > 1
        if tuple(pos) == d:
            return np.array(out, dtype=np.int64).reshape(-1, 3), tie
        out.append(tuple(pos))
    raise AssertionError(f"the walk along {d} did not arrive")


def _lit(solid, v, d):
    """Per pair (rows of v and d): no solid voxel before the lamp; and whether its walk ties."""
    dims = solid.shape
    lit, ties = np.ones(len(v), dtype=bool), np.zeros(len(v), dtype=bool)
    absd, sign = np.abs(d), np.sign(d)
    for lo in range(0, len(v), 20000):
        rows = range(lo, min(lo + 20000, len(v)))
        walks = [walk(tuple(int(c) for c in absd[i])) for i in rows]
        ties[lo:lo + len(walks)] = [w[1] for w in walks]
        lens = np.array([len(w[0]) for w in walks])
        if lens.sum() == 0:
            continue
        pair = np.repeat(np.arange(lo, lo + len(walks)), lens)
        pos = v[pair] + np.concatenate([w[0] for w in walks]) * sign[pair]
        inside = np.all((pos >= 0) & (pos < np.array(dims)), axis=1)
        hit = np.zeros(len(pos), dtype=bool)
        hit[inside] = solid[pos[inside, 0], pos[inside, 1], pos[inside, 2]]   # outside the world is air: the walk goes on
        lit[np.unique(pair[hit])] = False
    return lit, ties


def lamp_sum(solid, p, lamps):
    """-> (int64 volume: the sum of term_l over the lamps for every solid voxel inside the clipped box, 0 elsewhere;
    dict(lit: voxels with a non-zero sum, shadowed: pairs with d2 < r2 and facing > 0 that are shadowed, ties: pairs in range whose walk passes
    exactly through an edge or corner))."""
    dims = solid.shape
    total = np.zeros(dims, dtype=np.int64)
    stats = dict(lit=0, shadowed=0, ties=0)
    box = lightmodel.clip_box(dims, p["box_min"], p["box_max"])
    if box is None or not lamps:
        return total, stats
    lo, hi = box
    mask = np.zeros(dims, dtype=bool)
    inside = tuple(slice(lo[a], hi[a]) for a in range(3))
    mask[inside] = solid[inside]
    voxels = np.stack(np.nonzero(mask), axis=1).astype(np.int64)
    one = np.pad(solid, 1, constant_values=False)
    for l in lamps:
        d = np.array(l["pos"], dtype=np.int64) - voxels
        d2, r2 = (d * d).sum(axis=1), l["radius"] ** 2
        near = (d2 > 0) & (d2 < r2)
        v, d, d2 = voxels[near], d[near], d2[near]
        if len(v) == 0:
            continue
        facing = np.zeros(len(v), dtype=np.int64)
        for a in range(3):
            n = v + 1
            n[:, a] += np.sign(d[:, a])
            facing += np.abs(d[:, a]) * (d[:, a] != 0) * ~one[n[:, 0], n[:, 1], n[:, 2]]
        den = np.abs(d).sum(axis=1)
        lit, ties = _lit(solid, v, d)
        term = np.where(lit, l["level"] * (r2 - d2) * facing // (r2 * den), 0)
        np.add.at(total, (v[:, 0], v[:, 1], v[:, 2]), term)
        stats["shadowed"] += int(((facing > 0) & ~lit).sum())
        stats["ties"] += int(ties.sum())
    stats["lit"] = int((total > 0).sum())
    return total, stats


def shades(solid, p, lamps, total=None):
    """(`total`: what lamp_sum gave for the same arguments, when the caller has it.)  min(255, floor + sky + sun + lamps).  lightmodel.shades gives min(255, floor + sky + sun); min(255, min(255, a) + b) = min(255, a + b), b >= 0."""
    mask, shade = lightmodel.shades(solid, p)
    if total is None:
        total, _ = lamp_sum(solid, p, lamps)
    shade = np.minimum(255, shade + total)
    shade[~mask] = 0
    return mask, shade


def light(solid, colour, p, lamps, total=None):
    mask, shade = shades(solid, p, lamps, total)
    return lightmodel.apply(colour, mask, shade, p["target"])
