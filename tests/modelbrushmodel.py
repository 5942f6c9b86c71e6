"""An independent numpy model of cvxd_models_brush (include/cpuvox_gpu_model_brush.h), written from the contract alone: the SEQUENTIAL definition,
a stroke at a time and a voxel at a time.  It knows nothing about spans, columns, keys or waves: a stroke is tests/shapemodel.py's predicate
evaluated at every voxel of an instance's box (no footprint, no cull), the map tests/modelsmodel.py's, and a later stroke sees the arrays as the
earlier strokes left them.

A model is (argb, mask), arrays of shape (X, Z, Y) or None; an instance a dict as modelsmodel.from_struct gives; strokes as
cpuvox_amd.gpu.strokes_array takes them.
  brush(models, instances, strokes) -> (the models after the call, the model results as RESULT_DTYPE, the instance results as
                                        INSTANCE_DTYPE, the summary dict)
  jobs(instances, strokes)          -> the summary's `jobs`: the columns of the instances whose box meets the box around all strokes' footprints
  mass(result)                      -> (centre, inertia) in float64, cvx_lifted_piece_mass' formula with min = 0"""
from __future__ import annotations

import numpy as np

import modelsmodel
import shapemodel

RESULT_DTYPE = np.dtype([("voxels", "<i8"), ("carved", "<i8"), ("painted", "<i8"), ("sum", "<u8", 3), ("moment", "<u8", 6), ("min", "<i4", 3), ("max", "<i4", 3),
                         ("pad_", "<i4", 2)])
INSTANCE_DTYPE = np.dtype([("carved", "<i8"), ("painted", "<i8")])
SUMMARY_NAMES = ("carved", "painted", "models", "jobs")
MASK = (1 << 64) - 1


def _is_set(model):
    argb, mask = model
    return (np.asarray(mask) != 0) if mask is not None else (np.asarray(argb) != 0)


def _images(model, instance):
    """Over the instance's box, (x, y, z): whether a voxel's image lies in the model, and the image's index into the (X, Z, Y) arrays."""
    lo, hi = instance["box_min"], instance["box_max"]
    shape = (model[0] if model[0] is not None else model[1]).shape
    size = (shape[0], shape[2], shape[1])
    grid = np.meshgrid(*[np.arange(lo[i], hi[i], dtype=np.int64) for i in range(3)], indexing="ij")
    src = modelsmodel.apply_map(instance["m"], instance["t"], np.stack(grid, axis=-1))
    inside = np.ones(grid[0].shape, dtype=bool)
    for i in range(3):
        inside &= (src[..., i] >= 0) & (src[..., i] < size[i])
    sx, sy, sz = [np.where(inside, src[..., i], 0) for i in range(3)]
    return grid, inside, (sx, sz, sy)


def _holds(stroke, grid):
    """The stroke's predicate at every voxel of the grid.  A voxel outside the footprint box of include/cpuvox_gpu.h is outside the stroke; the
    products are formed for the others only (a voxel outside stands in as the stroke's own a), which keeps them in int64, as
    shapemodel.stroke_mask does."""
    _, shape, a, b, r, _ = shapemodel._fields(stroke)
    lo, hi = _footprint(stroke)
    near = np.ones(grid[0].shape, dtype=bool)
    for i in range(3):
        near &= (grid[i] >= lo[i]) & (grid[i] < hi[i])
    x, y, z = [np.where(near, grid[i], a[i]) for i in range(3)]
    return near & np.asarray(shapemodel._predicate(shape, a, b, r, x, y, z), dtype=bool)


def _footprint(stroke):
    _, shape, a, b, r, _ = shapemodel._fields(stroke)
    if shape == shapemodel.BOX:
        return list(a), list(b)
    if shape == shapemodel.CAPSULE:
        return [min(a[i], b[i]) - r for i in range(3)], [max(a[i], b[i]) + r + 1 for i in range(3)]
    radii = b if shape == shapemodel.ELLIPSOID else [r, r, r]
    return [a[i] - radii[i] for i in range(3)], [a[i] + radii[i] + 1 for i in range(3)]


def jobs(instances, strokes):
    boxes = [_footprint(s) for s in strokes]
    lo = [min(b[0][i] for b in boxes) for i in range(3)]
    hi = [max(b[1][i] for b in boxes) for i in range(3)]
    total = 0
    for inst in instances:
        if all(lo[i] < inst["box_max"][i] and hi[i] > inst["box_min"][i] for i in range(3)):
            total += (inst["box_max"][0] - inst["box_min"][0]) * (inst["box_max"][2] - inst["box_min"][2])
    return total


def brush(models, instances, strokes):
    after = [(None if a is None else np.array(a, dtype=np.uint32), None if m is None else np.array(np.asarray(m) != 0)) for a, m in models]
    strokes = list(strokes)
    ops = [shapemodel._fields(s)[0] for s in strokes]
    colours = [shapemodel._fields(s)[5] for s in strokes]
    assert all(op in (shapemodel.CARVE, shapemodel.PAINT) for op in ops) and all(c != 0 for op, c in zip(ops, colours) if op == shapemodel.PAINT)
    placed = [_images(after[inst["model"]], inst) for inst in instances]
    masks = [[_holds(s, grid) for s in strokes] for grid, _, _ in placed]  # (a stroke's shape does not change during the call)

    # the instance results: B_k as it is before the call
    hit = np.zeros(len(instances), dtype=INSTANCE_DTYPE)
    for k, (inst, (grid, inside, at)) in enumerate(zip(instances, placed)):
        model = after[inst["model"]]
        body = inside & _is_set(model)[at]
        carve = np.zeros(body.shape, dtype=bool)
        paint = np.zeros(body.shape, dtype=bool)
        for j, op in enumerate(ops):
            if op == shapemodel.CARVE:
                carve |= masks[k][j]
            elif model[0] is not None:
                paint |= masks[k][j]
        hit[k]["carved"] = int((body & carve).sum())
        hit[k]["painted"] = int((body & ~carve & paint).sum())

    # the strokes in order; a later stroke sees what the earlier ones did
    before = [int(_is_set(m).sum()) for m in after]
    touched = [np.zeros((m[0] if m[0] is not None else m[1]).shape, dtype=bool) for m in after]
    for j, (op, colour) in enumerate(zip(ops, colours)):
        for k, (inst, (grid, inside, at)) in enumerate(zip(instances, placed)):
            g = inst["model"]
            argb, mask = after[g]
            if op == shapemodel.PAINT and argb is None:
                continue
            body = inside & _is_set(after[g])[at] & masks[k][j]
            where = tuple(a[body] for a in at)
            if op == shapemodel.CARVE:
                if mask is not None:
                    mask[where] = False
                if argb is not None:
                    argb[where] = 0
            else:
                argb[where] = np.uint32(colour)
                touched[g][where] = True

    results = np.zeros(len(after), dtype=RESULT_DTYPE)
    for g, model in enumerate(after):
        is_set = _is_set(model)
        x, z, y = [c.astype(object) for c in np.nonzero(is_set)]  # (Python integers: the sums are modulo 2^64 by the contract, not by accident)
        r = results[g]
        r["voxels"] = len(x)
        r["carved"] = before[g] - len(x)
        r["painted"] = int((touched[g] & is_set).sum())
        r["sum"] = [int(v.sum()) & MASK if len(v) else 0 for v in (x, y, z)]
        r["moment"] = [int((p * q).sum()) & MASK if len(p) else 0 for p, q in ((x, x), (y, y), (z, z), (x, y), (y, z), (z, x))]
        if len(x):
            r["min"] = [int(v.min()) for v in (x, y, z)]
            r["max"] = [int(v.max()) + 1 for v in (x, y, z)]
    summary = dict(carved=int(results["carved"].sum()), painted=int(results["painted"].sum()),
                   models=int(((results["carved"] + results["painted"]) > 0).sum()), jobs=jobs(instances, strokes))
    return after, results, hit, summary


def mass(result):
    """include/cpuvox_gpu_lift.h's formula on { voxels, min = 0, sum, moment }, every operation rounded once."""
    n = float(int(result["voxels"]))
    s = [float(int(v)) for v in result["sum"]]
    m = [float(int(v)) for v in result["moment"]]
    c = [v / n for v in s]
    centre = np.array([(0.0 + c[a]) + 0.5 for a in range(3)])
    q = [m[a] - s[a] * c[a] for a in range(3)]
    own = n / 3.0
    inertia = [(q[1] + q[2]) + own, (q[2] + q[0]) + own, (q[0] + q[1]) + own] + [-(m[3 + k] - s[k] * c[(k + 1) % 3]) for k in range(3)]
    return centre, np.array(inertia)
