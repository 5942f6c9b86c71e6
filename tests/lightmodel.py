"""An independent dense model of cvx_world_light (include/cpuvox_gpu.h), written from the contract alone: the sky term by shifting a padded
boolean volume, the shadow walk's voxel sequence from fractions.Fraction (one sequence serves every voxel: it depends on sunDir only), facing and
the bake in numpy.

params(...) -> a dict of the call's parameters; shades(solid, p) -> (mask of the lit voxels, their shade volume);
light(solid, colour, p) -> the new colour volume; rectangle(p, dims, level_count) -> the call's rectangle."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

TO_RGB, TO_ALPHA = 0, 1
DIRECTIONS = [(dx, dy, dz) for dy in (0, 1) for dx in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def params(box_min, box_max, sun_dir=(0, 0, 0), sun_level=0, sun_range=0, sky_level=0, sky_range=0, floor_level=0, target=TO_RGB):
    return dict(box_min=[int(v) for v in box_min], box_max=[int(v) for v in box_max], sun_dir=[int(v) for v in sun_dir], sun_level=int(sun_level),
                sun_range=int(sun_range), sky_level=int(sky_level), sky_range=int(sky_range), floor_level=int(floor_level), target=int(target))


def words(p):
    """The 16 int32 words of cvx_light_params."""
    return [*p["box_min"], *p["box_max"], *p["sun_dir"], p["sun_level"], p["sun_range"], p["sky_level"], p["sky_range"], p["floor_level"], p["target"], 0]


def clip_box(dims, box_min, box_max):
    lo = [max(int(box_min[a]), 0) for a in range(3)]
    hi = [min(int(box_max[a]), dims[a]) for a in range(3)]
    return (lo, hi) if all(lo[a] < hi[a] for a in range(3)) else None


def rectangle(p, dims, level_count):
    box = clip_box(dims, p["box_min"], p["box_max"])
    if box is None:
        return None
    lo, hi = box
    m = (1 << level_count) - 1
    x0, z0 = lo[0] & ~m, lo[2] & ~m
    x1, z1 = min((hi[0] + m) & ~m, dims[0]), min((hi[2] + m) & ~m, dims[2])
    return x0, z0, x1 - x0, z1 - z0


def walk_offsets(sun_dir, sun_range, dims):
    """The voxels the ray from a voxel's centre along sun_dir reaches, relative to the voxel: axis i crosses its k-th plane at (2k - 1) / |S_i|,
    all axes with the smallest pending parameter advance together.  Stops where every start inside the world has left it."""
    k, pos, out = [1, 1, 1], [0, 0, 0], []
    for _ in range(sun_range):
        pending = {a: Fraction(2 * k[a] - 1, abs(sun_dir[a])) for a in range(3) if sun_dir[a] != 0}
        t = min(pending.values())
        for a, ta in pending.items():
            if ta == t:
                pos[a] += 1 if sun_dir[a] > 0 else -1
                k[a] += 1
        out.append(tuple(pos))
        if any(abs(pos[a]) >= dims[a] for a in range(3)):
            break
    return out


def shades(solid, p):
    dims = solid.shape
    mask = np.zeros(dims, dtype=bool)
    shade = np.zeros(dims, dtype=np.int64)
    box = clip_box(dims, p["box_min"], p["box_max"])
    if box is None:
        return mask, shade
    lo, hi = box
    inside = tuple(slice(lo[a], hi[a]) for a in range(3))
    mask[inside] = solid[inside]
    size = [hi[a] - lo[a] for a in range(3)]
    # sky: the padded volume shifted by s * d
    r = p["sky_range"]
    sky = np.zeros(size, dtype=np.int64)
    padded = np.pad(solid, r, constant_values=False)
    for d in DIRECTIONS:
        is_open = np.ones(size, dtype=bool)
        for s in range(1, r + 1):
            is_open &= ~padded[tuple(slice(lo[a] + r + s * d[a], hi[a] + r + s * d[a]) for a in range(3))]
        sky += (2 if d[1] == 1 else 1) * is_open
    total = p["floor_level"] + p["sky_level"] * sky // 26
    # sun
    sun = p["sun_dir"]
    if any(sun):
        one = np.pad(solid, 1, constant_values=False)
        facing = np.zeros(size, dtype=np.int64)
        for a in range(3):
            if sun[a]:
                step = [0, 0, 0]
                step[a] = 1 if sun[a] > 0 else -1
                facing += abs(sun[a]) * ~one[tuple(slice(lo[b] + 1 + step[b], hi[b] + 1 + step[b]) for b in range(3))]
        den = sum(abs(v) for v in sun)
        vx, vy, vz = np.nonzero(mask)
        lit = np.ones(len(vx), dtype=bool)
        active = np.arange(len(vx))
        for off in walk_offsets(sun, p["sun_range"], dims):
            if len(active) == 0:
                break
            x, y, z = vx[active] + off[0], vy[active] + off[1], vz[active] + off[2]
            outside = (x < 0) | (x >= dims[0]) | (y < 0) | (y >= dims[1]) | (z < 0) | (z >= dims[2])
            hit = np.zeros(len(active), dtype=bool)
            hit[~outside] = solid[x[~outside], y[~outside], z[~outside]]
            lit[active[hit]] = False
            active = active[~outside & ~hit]
        lit_volume = np.zeros(dims, dtype=bool)
        lit_volume[vx[lit], vy[lit], vz[lit]] = True
        total = total + np.where(lit_volume[inside], p["sun_level"] * facing // den, 0)
    shade[inside] = np.minimum(255, total)
    shade[~mask] = 0
    return mask, shade


def apply(colour, mask, shade, target):
    """Colour words hold the bytes a, r, g, b: alpha is the low byte."""
    c = colour.astype(np.int64)
    if target == TO_ALPHA:
        out = (c & 0xFFFFFF00) | shade
    else:
        out = c & 0xFF
        for shift in (8, 16, 24):
            out |= ((((c >> shift) & 0xFF) * shade + 127) // 255) << shift
    return np.where(mask, out, c).astype(np.uint32)


def light(solid, colour, p):
    mask, shade = shades(solid, p)
    return apply(colour, mask, shade, p["target"])
