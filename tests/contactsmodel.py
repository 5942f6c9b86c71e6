"""An independent numpy model of cvxc_world_contacts / cvxc_contact_response (include/cpuvox_gpu_contacts.h), written from the contract alone.  It
knows nothing about runs, columns or waves: the world is a pair of (x, y, z) volumes, `solid` (bool) and `colour` (uint32, 0 for air), as in the
other models; Solid(v) outside it is tests/distancemodel.py's, the map tests/modelsmodel.py's.

A model is (argb, mask), arrays of shape (X, Z, Y) or None; an instance a dict as modelsmodel.from_struct gives.
  body(models, instance)                              -> the bool array of B_k over the instance's box, (x, y, z)
  contacts(solid, colour, models, instances, solid_outside) -> (results as RESULT_DTYPE, the full list of points as POINT_DTYPE, the summary dict)
  response(result)                                    -> (centre, normal, depth) in float64, the header's formula"""
from __future__ import annotations

import numpy as np

import distancemodel
import modelsmodel

RESULT_DTYPE = np.dtype([("voxels", "<i8"), ("overlap", "<i8"), ("points", "<i8"), ("firstPoint", "<i8"), ("sum", "<u8", 3), ("normal", "<i8", 3),
                         ("origin", "<i4", 3), ("min", "<i4", 3), ("max", "<i4", 3), ("pad_", "<i4")])
POINT_DTYPE = np.dtype([("voxel", "<i4", 3), ("instance", "<i4"), ("faces", "<i4"), ("argb", "<u4")])
SUMMARY_NAMES = ("touching", "overlap", "points", "voxels")


def body(models, instance):
    lo, hi = instance["box_min"], instance["box_max"]
    argb, mask = models[instance["model"]]
    shape = (argb if argb is not None else mask).shape  # (X, Z, Y)
    size = (shape[0], shape[2], shape[1])
    d = np.stack(np.meshgrid(*[np.arange(lo[i], hi[i], dtype=np.int64) for i in range(3)], indexing="ij"), axis=-1)
    src = modelsmodel.apply_map(instance["m"], instance["t"], d)
    inside = np.ones(d.shape[:-1], dtype=bool)
    for i in range(3):
        inside &= (src[..., i] >= 0) & (src[..., i] < size[i])
    sx, sy, sz = [np.where(inside, src[..., i], 0) for i in range(3)]
    is_set = (np.asarray(mask)[sx, sz, sy] != 0) if mask is not None else (np.asarray(argb)[sx, sz, sy] != 0)
    return inside & is_set


def contacts(solid, colour, models, instances, solid_outside):
    dims = solid.shape
    results = np.zeros(len(instances), dtype=RESULT_DTYPE)
    lists = []
    for k, inst in enumerate(instances):
        lo, hi = [int(v) for v in inst["box_min"]], [int(v) for v in inst["box_max"]]
        b = body(models, inst)
        world = distancemodel.volume(solid, [v - 1 for v in lo], [v + 1 for v in hi], solid_outside)  # Solid over the box and a voxel around it
        inner = (slice(1, -1),) * 3
        o = b & world[inner]
        faces = np.zeros(b.shape, dtype=np.int32)
        r = results[k]
        r["voxels"], r["overlap"], r["origin"] = int(b.sum()), int(o.sum()), lo
        for f in range(6):
            axis, step = f // 2, (1 if f % 2 else -1)
            shifted = [slice(1, -1)] * 3
            shifted[axis] = slice(1 + step, world.shape[axis] - 1 + step)
            open_face = o & ~world[tuple(shifted)]
            faces |= open_face.astype(np.int32) << f
            r["normal"][axis] += step * int(open_face.sum())
        x, y, z = np.nonzero(o)
        if len(x):
            r["sum"] = [int(x.sum()), int(y.sum()), int(z.sum())]
            r["min"] = [lo[0] + int(x.min()), lo[1] + int(y.min()), lo[2] + int(z.min())]
            r["max"] = [lo[0] + int(x.max()) + 1, lo[1] + int(y.max()) + 1, lo[2] + int(z.max()) + 1]
        x, y, z = np.nonzero(o & (faces != 0))
        order = np.lexsort((-y, z, x))  # x ascending, then z ascending, then y descending
        x, y, z = x[order], y[order], z[order]
        points = np.zeros(len(x), dtype=POINT_DTYPE)
        wx, wy, wz = x + lo[0], y + lo[1], z + lo[2]
        points["voxel"] = np.stack([wx, wy, wz], axis=-1)
        points["instance"] = k
        points["faces"] = faces[x, y, z]
        in_world = (wx >= 0) & (wx < dims[0]) & (wy >= 0) & (wy < dims[1]) & (wz >= 0) & (wz < dims[2])
        points["argb"] = np.where(in_world, colour[np.where(in_world, wx, 0), np.where(in_world, wy, 0), np.where(in_world, wz, 0)], 0)
        r["points"] = len(points)
        r["firstPoint"] = sum(len(p) for p in lists)
        lists.append(points)
    points = np.concatenate(lists) if lists else np.zeros(0, dtype=POINT_DTYPE)
    summary = dict(touching=int((results["overlap"] > 0).sum()), overlap=int(results["overlap"].sum()), points=len(points), voxels=int(results["voxels"].sum()))
    return results, points, summary


def response(result):
    """The header's formula, operation by operation, in float64."""
    n = np.float64(int(result["overlap"]))
    centre = np.array([(np.float64(int(result["origin"][a])) + np.float64(int(result["sum"][a])) / n) + 0.5 for a in range(3)])
    g = np.array([np.float64(int(result["normal"][a])) for a in range(3)])
    length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    normal = g / length if length > 0 else np.zeros(3)
    return centre, normal, (n / length if length > 0 else np.float64(0.0))
