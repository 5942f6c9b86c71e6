"""Test infrastructure: independent numpy models of cvx_world_brush and cvx_world_pick (include/cpuvox_gpu.h) on a dense voxel volume.

- apply_strokes: the strokes in order on a dense (solid, colour) volume, integer shapes.
- pick: a float64 3-D DDA over the dense volume (Amanatides & Woo, voxel by voxel; not the library's column walk), which also says whether a
  ray is resolved unambiguously: a ray is AMBIGUOUS when, on its way to the hit (or out of the world), two plane crossings of different axes lie
  within EPS voxel of each other and a voxel either order would enter first is solid (the ray passes a solid voxel's edge), when it enters
  the world within EPS of an edge of the world box, or when the hit lies within EPS of maxT.  A ray on a voxel plane that it never leaves (its
  direction 0 along that axis) is not ambiguous: the cube of voxel x is [x, x + 1), for the model and the library alike.  Distances are along the ray.
"""
from __future__ import annotations

import math

import numpy as np

EPS = 1e-4


def stroke_mask(stroke, shape):
    """bool[dx, dy, dz]: the voxels inside the stroke's shape, clipped to the volume."""
    dx, dy, dz = shape
    x = np.arange(dx, dtype=np.int64)[:, None, None]
    y = np.arange(dy, dtype=np.int64)[None, :, None]
    z = np.arange(dz, dtype=np.int64)[None, None, :]
    a, b = [int(v) for v in stroke["a"]], [int(v) for v in stroke["b"]]
    if int(stroke["shape"]) == 0:
        return (x >= a[0]) & (x < b[0]) & (y >= a[1]) & (y < b[1]) & (z >= a[2]) & (z < b[2])
    r = b[0]
    return (x - a[0]) ** 2 + (y - a[1]) ** 2 + (z - a[2]) ** 2 <= r * r


def apply_strokes(solid, colour, strokes):
    """In place: FILL -> solid with argb, CARVE -> air, PAINT -> argb on the solid voxels only."""
    for s in strokes:
        m = stroke_mask(s, solid.shape)
        op, argb = int(s["op"]), np.uint32(int(s["argb"]) & 0xFFFFFFFF)
        if op == 0:
            solid |= m
            colour[m] = argb
        elif op == 1:
            solid &= ~m
        else:
            colour[m & solid] = argb
    colour[~solid] = 0


def _face(axis, d):
    return 2 * axis + (0 if d > 0 else 1)


def pick(solid, colour, origin, direction, max_t):
    """-> (voxel, face, argb, t, ambiguous) for one ray; origin / direction / max_t as float32 values (the library's input)."""
    dims = solid.shape
    o = [float(np.float32(v)) for v in origin]
    d = [float(np.float32(v)) for v in direction]
    max_t = float(np.float32(max_t))
    length = math.sqrt(sum(v * v for v in d))
    miss = ((-1, -1, -1), -1, 0, max_t)
    t_enter, t_exit, axis_enter = 0.0, max_t, -1
    enters = []
    for a in range(3):
        if d[a] == 0.0:
            if not (0.0 <= o[a] < dims[a]):
                return miss + (False,)
            continue
        t0, t1 = (0.0 - o[a]) / d[a], (dims[a] - o[a]) / d[a]
        t0, t1 = min(t0, t1), max(t0, t1)
        enters.append(t0)
        if t0 > t_enter:
            t_enter, axis_enter = t0, a
        t_exit = min(t_exit, t1)
    if t_enter > t_exit:
        return miss + (abs(t_enter - t_exit) * length < EPS,)
    ambiguous = False
    if axis_enter >= 0:
        close = [t for t in enters if t > 0 and abs(t - t_enter) * length < EPS]
        ambiguous |= len(close) > 1
        p = [o[a] + t_enter * d[a] for a in range(3)]
        v = [min(max(int(math.floor(p[a])), 0), dims[a] - 1) for a in range(3)]
        face = _face(axis_enter, d[axis_enter])
    else:
        v = [min(int(math.floor(o[a])), dims[a] - 1) for a in range(3)]
        face = 6
    step = [1 if d[a] > 0 else -1 for a in range(3)]
    t_next = [((v[a] + (1 if d[a] > 0 else 0)) - o[a]) / d[a] if d[a] != 0.0 else math.inf for a in range(3)]
    t = t_enter

    def inside(w):
        return all(0 <= w[a] < dims[a] for a in range(3))

    while True:
        if solid[v[0], v[1], v[2]]:
            if t > max_t:
                return miss + (ambiguous or (t - max_t) * length < EPS,)
            ambiguous |= (max_t - t) * length < EPS and face != 6
            return (tuple(v), face, int(colour[v[0], v[1], v[2]]), 0.0 if face == 6 else t, ambiguous)
        order = sorted(range(3), key=lambda a: t_next[a])
        a, b = order[0], order[1]
        if t_next[a] > t_exit:
            return miss + (ambiguous or (t_next[a] - t_exit) * length < EPS,)
        if (t_next[b] - t_next[a]) * length < EPS and t_next[b] <= t_exit + EPS:
            for c in (a, b):  # the voxels either order enters first
                other = list(v)
                other[c] += step[c]
                if inside(other) and solid[other[0], other[1], other[2]]:
                    ambiguous = True
        v[a] += step[a]
        t = t_next[a]
        face = _face(a, d[a])
        t_next[a] = ((v[a] + (1 if d[a] > 0 else 0)) - o[a]) / d[a]
        if not inside(v):
            return miss + (ambiguous,)


def pick_many(solid, colour, origins, directions, max_t):
    """-> voxel int32[N, 3], face int32[N], argb uint32[N], t float64[N], ambiguous bool[N]."""
    n = len(origins)
    max_t = np.broadcast_to(np.asarray(max_t, dtype=np.float32), (n,))
    vox = np.zeros((n, 3), dtype=np.int32)
    face = np.zeros(n, dtype=np.int32)
    argb = np.zeros(n, dtype=np.uint32)
    t = np.zeros(n, dtype=np.float64)
    amb = np.zeros(n, dtype=bool)
    for i in range(n):
        vox[i], face[i], argb[i], t[i], amb[i] = pick(solid, colour, origins[i], directions[i], max_t[i])
    return vox, face, argb, t, amb


def random_rays(rng, dims, n):
    """Rays from inside and outside the world, axis-aligned ones, rays along column boundaries, and maxT cut-offs."""
    dims = np.array(dims, dtype=np.float64)
    o = rng.uniform(-0.3, 1.3, size=(n, 3)) * dims
    target = rng.uniform(0.0, 1.0, size=(n, 3)) * dims
    d = target - o
    kind = rng.integers(0, 6, size=n)
    axis = rng.integers(0, 3, size=n)
    for i in np.nonzero(kind == 1)[0]:  # axis-aligned
        d[i] = 0.0
        d[i, axis[i]] = rng.choice([-1.0, 1.0]) * rng.uniform(0.5, 3.0)
    for i in np.nonzero(kind == 2)[0]:  # inside the world, along a column boundary (x or z integral; y direction random)
        o[i] = rng.uniform(0.0, 1.0, size=3) * dims
        o[i, 0 if axis[i] != 2 else 2] = float(rng.integers(1, int(dims[0 if axis[i] != 2 else 2])))
        d[i, 0 if axis[i] != 2 else 2] = 0.0
    for i in np.nonzero(kind == 3)[0]:  # inside the world
        o[i] = rng.uniform(0.0, 1.0, size=3) * dims
    max_t = np.where(kind == 4, rng.uniform(0.05, 0.6, size=n), 1e4).astype(np.float32)
    d[np.all(d == 0.0, axis=1)] = (0.0, -1.0, 0.0)
    return o.astype(np.float32), d.astype(np.float32), max_t


def compare_picks(hits, model, label):
    """hits (PICK_HIT_DTYPE) against pickmodel.pick_many's output: exact on the unambiguous rays.  -> the unambiguous fraction."""
    vox, face, argb, t, amb = model
    ok = ~amb
    bad = ok & ((hits["voxel"] != vox).any(axis=1) | (hits["face"] != face) | (hits["argb"] != argb) |
                ~np.isclose(hits["t"].astype(np.float64), t, rtol=1e-5, atol=1e-5))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {int(ok.sum())} unambiguous rays differ; first #{i}: got {hits[i]}, "
                             f"want voxel {vox[i].tolist()} face {face[i]} argb {argb[i]:#x} t {t[i]}")
    return float(ok.mean())
