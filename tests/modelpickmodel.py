"""An independent numpy model of cvxq_model_pick (include/cpuvox_gpu_model_pick.h), written from the contract alone.  It knows nothing about layers,
jobs or waves: per instance the body is tests/contactsmodel.py's bool array over the instance's box, and the ray is walked through that dense
volume by the float64 3-D DDA of tests/pickmodel.py (Amanatides & Woo with divisions, voxel by voxel), in the box's own coordinates: the
float32 inputs are taken to float64 first and the box's offset is subtracted in float64, never recast to float32.

A ray is AMBIGUOUS (pickmodel's rule, EPS = 1e-4 voxel along the ray) when, against any instance, two plane crossings of different axes lie within
EPS of each other next to a body voxel, it enters the box within EPS of one of the box's edges, or a hit lies within EPS of maxT; and also when
its two nearest bodies' hits lie within EPS of each other.

A model is (argb, mask), arrays of shape (X, Z, Y) or None; an instance a dict as modelsmodel.from_struct gives.
  pick_many(models, instances, origins, directions, max_t) -> HITS (MODEL_HIT's fields, t in float64), ambiguous bool[N]"""
from __future__ import annotations

import math

import numpy as np

import contactsmodel
import modelsmodel
from pickmodel import EPS

HIT_DTYPE = np.dtype([("voxel", "<i4", 3), ("face", "<i4"), ("argb", "<u4"), ("t", "<f8"), ("instance", "<i4"), ("modelVoxel", "<i4", 3)])


def _face(axis, d):
    return 2 * axis + (0 if d > 0 else 1)


def pick_box(solid, o, d, max_t):
    """The first True voxel of `solid` (x, y, z) along the ray o + t d, all float64, t in [0, max_t]: (voxel or None, face, t, ambiguous)."""
    dims = solid.shape
    length = math.sqrt(sum(v * v for v in d))
    t_enter, t_exit, axis_enter = 0.0, max_t, -1
    enters = []
    for a in range(3):
        if d[a] == 0.0:
            if not (0.0 <= o[a] < dims[a]):
                return None, -1, max_t, False
            continue
        t0, t1 = (0.0 - o[a]) / d[a], (dims[a] - o[a]) / d[a]
        t0, t1 = min(t0, t1), max(t0, t1)
        enters.append(t0)
        if t0 > t_enter:
            t_enter, axis_enter = t0, a
        t_exit = min(t_exit, t1)
    if t_enter > t_exit:
        return None, -1, max_t, abs(t_enter - t_exit) * length < EPS
    ambiguous = False
    if axis_enter >= 0:
        ambiguous |= len([t for t in enters if t > 0 and abs(t - t_enter) * length < EPS]) > 1
        v = [min(max(int(math.floor(o[a] + t_enter * d[a])), 0), dims[a] - 1) for a in range(3)]
        face = _face(axis_enter, d[axis_enter])
    else:
        v = [min(max(int(math.floor(o[a])), 0), dims[a] - 1) for a in range(3)]
        face = 6
    step = [1 if d[a] > 0 else -1 for a in range(3)]
    t_next = [((v[a] + (1 if d[a] > 0 else 0)) - o[a]) / d[a] if d[a] != 0.0 else math.inf for a in range(3)]
    t = t_enter

    def inside(w):
        return all(0 <= w[a] < dims[a] for a in range(3))

    while True:
        if solid[v[0], v[1], v[2]]:
            ambiguous |= (max_t - t) * length < EPS and face != 6
            return tuple(v), face, t, ambiguous
        order = sorted(range(3), key=lambda a: t_next[a])
        a, b = order[0], order[1]
        if t_next[a] > t_exit or t_next[a] == math.inf:
            return None, -1, max_t, ambiguous or (t_next[a] - t_exit) * length < EPS
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
            return None, -1, max_t, ambiguous


def pick_many(models, instances, origins, directions, max_t):
    n = len(origins)
    origins, directions = np.asarray(origins, dtype=np.float32), np.asarray(directions, dtype=np.float32)
    max_t = np.broadcast_to(np.asarray(max_t, dtype=np.float32), (n,))
    bodies = [contactsmodel.body(models, inst) for inst in instances]
    hits = np.zeros(n, dtype=HIT_DTYPE)
    amb = np.zeros(n, dtype=bool)
    for i in range(n):
        o = [float(v) for v in origins[i]]
        d = [float(v) for v in directions[i]]
        limit = float(max_t[i])
        hits[i] = ((-1, -1, -1), -1, 0, limit, -1, (-1, -1, -1))
        if not all(abs(v) < 1e30 for v in o + d) or not limit >= 0.0:  # (a NaN fails every comparison)
            continue
        length = math.sqrt(sum(v * v for v in d))
        found = []
        for k, inst in enumerate(instances):
            lo = inst["box_min"]
            v, face, t, ambiguous = pick_box(bodies[k], [o[a] - float(lo[a]) for a in range(3)], d, limit)
            amb[i] |= ambiguous
            if v is not None:
                found.append((t, k, [v[a] + lo[a] for a in range(3)], face))
        if not found:
            continue
        found.sort(key=lambda f: (f[0], f[1]))
        t, k, v, face = found[0]
        if len(found) > 1 and (found[1][0] - t) * length < EPS:
            amb[i] = True
        inst = instances[k]
        s = [int(c) for c in modelsmodel.apply_map(inst["m"], inst["t"], v)]
        argb = models[inst["model"]][0]
        hits[i] = (v, face, 0 if argb is None else int(argb[s[0], s[2], s[1]]), t, k, s)
    return hits, amb


def compare(got, model, label):
    """got (gpu.MODEL_HIT_DTYPE) against pick_many's output: exact voxel, face, argb, instance and modelVoxel, t within pickmodel.compare_picks'
    tolerance, on the unambiguous rays.  -> the unambiguous fraction."""
    want, amb = model
    ok = ~amb
    bad = ok & ((got["voxel"] != want["voxel"]).any(axis=1) | (got["face"] != want["face"]) | (got["argb"] != want["argb"]) | (got["instance"] != want["instance"]) |
                (got["modelVoxel"] != want["modelVoxel"]).any(axis=1) | ~np.isclose(got["t"].astype(np.float64), want["t"], rtol=1e-5, atol=1e-5))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{label}: {int(bad.sum())} of {int(ok.sum())} unambiguous rays differ; first #{i}: got {got[i]}, want {want[i]}")
    return float(ok.mean())
