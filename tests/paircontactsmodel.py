"""An independent numpy model of cvxp_model_contacts / cvxp_box_pairs / cvxp_pair_response (include/cpuvox_gpu_pair_contacts.h), written from the
contract alone.  It knows nothing about columns, jobs or waves: a body is tests/contactsmodel.py's bool volume over the instance's own box, laid
into whatever region is asked for (False outside the box); the map is tests/modelsmodel.py's.

A model is (argb, mask), arrays of shape (X, Z, Y) or None; an instance a dict as modelsmodel.from_struct gives.
  body_in(models, instance, lo, hi)   -> the bool array of B_k over [lo, hi), (x, y, z)
  contacts(models, instances, pairs)  -> (results as RESULT_DTYPE, the full list of points as POINT_DTYPE, the summary dict)
  box_pairs(instances, margin)        -> the (n, 2) int32 array, by a double loop
  response(result, which)             -> (centre, normal, depth) in float64, the header's formula"""
from __future__ import annotations

import numpy as np

import contactsmodel
import modelsmodel

RESULT_DTYPE = np.dtype([("overlap", "<i8"), ("points", "<i8"), ("firstPoint", "<i8"), ("sum", "<u8", 3), ("pushA", "<i8", 3), ("pushB", "<i8", 3),
                         ("origin", "<i4", 3), ("min", "<i4", 3), ("max", "<i4", 3), ("a", "<i4"), ("b", "<i4"), ("pad_", "<i4")])
POINT_DTYPE = np.dtype([("voxel", "<i4", 3), ("pair", "<i4"), ("facesA", "<i4"), ("facesB", "<i4"), ("argbA", "<u4"), ("argbB", "<u4")])
SUMMARY_NAMES = ("touching", "overlap", "points", "jobs")


def body_in(models, instance, lo, hi, own=None):
    """B_k over [lo, hi): the body over its own box (`own`, if the caller has it already), False everywhere else."""
    out = np.zeros([max(int(hi[i]) - int(lo[i]), 0) for i in range(3)], dtype=bool)
    b_lo, b_hi = [int(v) for v in instance["box_min"]], [int(v) for v in instance["box_max"]]
    c_lo, c_hi = [max(int(lo[i]), b_lo[i]) for i in range(3)], [min(int(hi[i]), b_hi[i]) for i in range(3)]
    if any(c_lo[i] >= c_hi[i] for i in range(3)):
        return out
    own = contactsmodel.body(models, instance) if own is None else own
    out[tuple(slice(c_lo[i] - int(lo[i]), c_hi[i] - int(lo[i])) for i in range(3))] = own[tuple(slice(c_lo[i] - b_lo[i], c_hi[i] - b_lo[i]) for i in range(3))]
    return out


def _colours(model, instance, voxels):
    argb = model[0]
    if argb is None or not len(voxels):
        return np.zeros(len(voxels), dtype=np.uint32)
    s = modelsmodel.apply_map(instance["m"], instance["t"], voxels.astype(np.int64))
    return np.asarray(argb, dtype=np.uint32)[s[:, 0], s[:, 2], s[:, 1]]


def contacts(models, instances, pairs):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    results = np.zeros(len(pairs), dtype=RESULT_DTYPE)
    own = {}
    lists, jobs, listed = [], 0, 0
    for p, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        ia, ib = instances[a], instances[b]
        lo = [max(int(ia["box_min"][i]), int(ib["box_min"][i])) for i in range(3)]
        hi = [min(int(ia["box_max"][i]), int(ib["box_max"][i])) for i in range(3)]
        r = results[p]
        r["origin"], r["a"], r["b"], r["firstPoint"] = lo, a, b, listed
        if any(lo[i] >= hi[i] for i in range(3)):
            continue
        jobs += (hi[0] - lo[0]) * (hi[2] - lo[2])
        for k in (a, b):
            if k not in own:
                own[k] = contactsmodel.body(models, instances[k])
        wide_lo, wide_hi = [v - 1 for v in lo], [v + 1 for v in hi]  # X_p and a voxel around it
        wa, wb = body_in(models, ia, wide_lo, wide_hi, own[a]), body_in(models, ib, wide_lo, wide_hi, own[b])
        inner = (slice(1, -1),) * 3
        o = wa[inner] & wb[inner]
        faces = [np.zeros(o.shape, dtype=np.int32), np.zeros(o.shape, dtype=np.int32)]
        for f in range(6):
            axis, step = f // 2, (1 if f % 2 else -1)
            shifted = [slice(1, -1)] * 3
            shifted[axis] = slice(1 + step, wa.shape[axis] - 1 + step)
            open_a, open_b = o & ~wa[tuple(shifted)], o & ~wb[tuple(shifted)]
            faces[0] |= open_a.astype(np.int32) << f
            faces[1] |= open_b.astype(np.int32) << f
            r["pushB"][axis] += step * int(open_a.sum())
            r["pushA"][axis] += step * int(open_b.sum())
        r["overlap"] = int(o.sum())
        x, y, z = np.nonzero(o)
        if len(x):
            r["sum"] = [int(x.sum()), int(y.sum()), int(z.sum())]
            r["min"] = [lo[0] + int(x.min()), lo[1] + int(y.min()), lo[2] + int(z.min())]
            r["max"] = [lo[0] + int(x.max()) + 1, lo[1] + int(y.max()) + 1, lo[2] + int(z.max()) + 1]
        x, y, z = np.nonzero(o & ((faces[0] | faces[1]) != 0))
        order = np.lexsort((-y, z, x))  # x ascending, then z ascending, then y descending
        x, y, z = x[order], y[order], z[order]
        points = np.zeros(len(x), dtype=POINT_DTYPE)
        points["voxel"] = np.stack([x + lo[0], y + lo[1], z + lo[2]], axis=-1)
        points["pair"] = p
        points["facesA"], points["facesB"] = faces[0][x, y, z], faces[1][x, y, z]
        points["argbA"] = _colours(models[ia["model"]], ia, points["voxel"])
        points["argbB"] = _colours(models[ib["model"]], ib, points["voxel"])
        r["points"] = len(points)
        listed += len(points)
        lists.append(points)
    points = np.concatenate(lists) if lists else np.zeros(0, dtype=POINT_DTYPE)
    summary = dict(touching=int((results["overlap"] > 0).sum()), overlap=int(results["overlap"].sum()), points=len(points), jobs=jobs)
    return results, points, summary


def box_pairs(instances, margin=0):
    """Every (a, b), a < b, whose boxes widened by `margin` on every side intersect: the double loop."""
    out = []
    for a in range(len(instances)):
        for b in range(a + 1, len(instances)):
            ia, ib = instances[a], instances[b]
            if all(max(int(ia["box_min"][i]), int(ib["box_min"][i])) - margin < min(int(ia["box_max"][i]), int(ib["box_max"][i])) + margin for i in range(3)):
                out.append((a, b))
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)


def response(result, which):
    """The header's formula, operation by operation, in float64."""
    n = np.float64(int(result["overlap"]))
    centre = np.array([(np.float64(int(result["origin"][a])) + np.float64(int(result["sum"][a])) / n) + 0.5 for a in range(3)])
    push = result["pushA" if which == 0 else "pushB"]
    g = np.array([np.float64(int(push[a])) for a in range(3)])
    length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    normal = g / length if length > 0 else np.zeros(3)
    return centre, normal, (n / length if length > 0 else np.float64(0.0))
