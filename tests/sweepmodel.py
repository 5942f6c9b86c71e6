"""An independent numpy model of cvxs_world_sweep / cvxs_sweep_offset / cvxs_instance_moved (include/cpuvox_gpu_sweep.h), written from the
contract alone.  It knows nothing about stations, columns or waves: the path comes from sorting the steps' (parameter, axis) keys as
fractions.Fraction, and the sweep calls tests/contactsmodel.py's contacts on I + o_j for j = 0, 1, ... until it finds an overlap.

  path(motion)                     -> [(o_j as a tuple, the axis of step j)] for j = 0 .. n, axis -1 for j = 0
  moved(instance, offset)          -> the instance dict (modelsmodel.from_struct's) of I + o
  sweep(solid, colour, models, instances, motions, solid_outside)
                                   -> (sweeps as RESULT_DTYPE, contact results, the full list of points, the summary dict without `jobs`)
  jobs(instances, motions)         -> the summary's `jobs`: sum of footprint * (|vx| + |vz| + 1)"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import contactsmodel

RESULT_DTYPE = np.dtype([("steps", "<i4"), ("hit", "<i4"), ("axis", "<i4"), ("sign", "<i4"), ("free", "<i4", 3), ("at", "<i4", 3), ("pad_", "<i4", 2)])
SUMMARY_NAMES = ("hits", "startsSolid", "jobs", "points")
MAX_MOTION = 4096


def path(motion):
    v = [int(c) for c in motion]
    keys = sorted((Fraction(2 * k - 1, 2 * abs(v[a])), a) for a in range(3) for k in range(1, abs(v[a]) + 1))
    o, out = [0, 0, 0], [((0, 0, 0), -1)]
    for _, a in keys:
        o[a] += 1 if v[a] > 0 else -1
        out.append((tuple(o), a))
    return out


def moved(instance, offset):
    o = [int(c) for c in offset]
    m = instance["m"]
    return dict(instance, box_min=[int(instance["box_min"][a]) + o[a] for a in range(3)], box_max=[int(instance["box_max"][a]) + o[a] for a in range(3)],
                t=[int(instance["t"][i]) - sum(int(m[i][a]) * o[a] for a in range(3)) for i in range(3)])


def _one(solid, colour, models, instance, motion, solid_outside):
    steps = path(motion)
    for j, (o, _) in enumerate(steps):
        results, _, _ = contactsmodel.contacts(solid, colour, models, [moved(instance, o)], solid_outside)
        if results["overlap"][0] > 0:
            return j, steps
    return -1, steps


def sweep(solid, colour, models, instances, motions, solid_outside):
    sweeps = np.zeros(len(instances), dtype=RESULT_DTYPE)
    touching, seen = [], {}
    for k, (inst, v) in enumerate(zip(instances, motions)):
        v = [int(c) for c in v]
        key = repr((inst["m"], inst["t"], inst["box_min"], inst["box_max"], inst["model"], v))  # (an instance's answer does not depend on the others)
        if key not in seen:
            seen[key] = _one(solid, colour, models, inst, v, solid_outside)
        hit, steps = seen[key]
        r = sweeps[k]
        r["steps"], r["hit"], r["axis"] = len(steps) - 1, hit, -1
        r["free"] = r["at"] = v if hit < 0 else (0, 0, 0)
        if hit > 0:
            r["at"], r["axis"] = steps[hit]
            r["free"] = steps[hit - 1][0]
            r["sign"] = 1 if v[r["axis"]] > 0 else -1
        touching.append(moved(inst, r["at"]))
    results, points, totals = contactsmodel.contacts(solid, colour, models, touching, solid_outside)
    return sweeps, results, points, dict(hits=int((sweeps["hit"] >= 0).sum()), startsSolid=int((sweeps["hit"] == 0).sum()), points=totals["points"])


def jobs(instances, motions):
    return sum((i["box_max"][0] - i["box_min"][0]) * (i["box_max"][2] - i["box_min"][2]) * (abs(int(v[0])) + abs(int(v[2])) + 1) for i, v in zip(instances, motions))
