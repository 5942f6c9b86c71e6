"""An independent numpy model of cvxm_pair_sweep (include/cpuvox_gpu_pair_sweep.h), written from the contract alone.  It knows nothing about
columns, windows or waves: the path is tests/sweepmodel.py's sorted fractions, a body is tests/contactsmodel.py's bool volume over the instance's
own box (the body rule of tests/paircontactsmodel.py), and the sweep lays body a, shifted by o_j, over body b for j = 0, 1, ... until the two
share a voxel.  The contacts are tests/paircontactsmodel.py's of the instance that sweepmodel.moved makes, which also checks, pose `at` by
pose `at`, that the shifted volume is the moved instance's body.

An instance is a dict as modelsmodel.from_struct gives.
  hit_of(body_a, box_a, body_b, box_b, steps) -> the least j whose pose overlaps, -1 for none
  sweep(models, instances, pairs, motions, want_contacts=True)
                                   -> (sweeps as RESULT_DTYPE, contacts as paircontactsmodel.RESULT_DTYPE or None, the summary dict with jobs)
  jobs(instances, pairs, motions)  -> the summary's `jobs`, by counting the coordinates of the header's R_c one by one"""
from __future__ import annotations

import numpy as np

import contactsmodel
import paircontactsmodel
import sweepmodel

RESULT_DTYPE = np.dtype([("sweep", sweepmodel.RESULT_DTYPE), ("a", "<i4"), ("b", "<i4")])
SUMMARY_NAMES = ("hits", "startsSolid", "jobs")


def _overlap(body_a, lo_a, body_b, lo_b, o):
    """Whether body a shifted by o and body b share a voxel: both volumes cut to the intersection of the shifted box of a and the box of b."""
    cut_a, cut_b = [], []
    for c in range(3):
        at = lo_a[c] + o[c]
        lo, hi = max(at, lo_b[c]), min(at + body_a.shape[c], lo_b[c] + body_b.shape[c])
        if lo >= hi:
            return False
        cut_a.append(slice(lo - at, hi - at))
        cut_b.append(slice(lo - lo_b[c], hi - lo_b[c]))
    return bool((body_a[tuple(cut_a)] & body_b[tuple(cut_b)]).any())


def hit_of(body_a, lo_a, body_b, lo_b, steps):
    for j, (o, _) in enumerate(steps):
        if _overlap(body_a, lo_a, body_b, lo_b, o):
            return j
    return -1


def _reach(a_lo, a_hi, b_lo, b_hi, v):
    """|R_c|: the u of [a_lo, a_hi) for which [min(u, u + v), max(u, u + v)] meets [b_lo, b_hi)."""
    return sum(1 for u in range(a_lo, a_hi) if max(u, u + v) >= b_lo and min(u, u + v) <= b_hi - 1)


def pair_jobs(ia, ib, v):
    r = [_reach(int(ia["box_min"][c]), int(ia["box_max"][c]), int(ib["box_min"][c]), int(ib["box_max"][c]), int(v[c])) for c in range(3)]
    return r[0] * r[2] if r[1] > 0 else 0


def jobs(instances, pairs, motions):
    return sum(pair_jobs(instances[int(a)], instances[int(b)], v) for (a, b), v in zip(np.asarray(pairs).reshape(-1, 2), motions))


def sweep(models, instances, pairs, motions, want_contacts=True):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    sweeps = np.zeros(len(pairs), dtype=RESULT_DTYPE)
    bodies, seen, count = {}, {}, 0
    for p, ((a, b), v) in enumerate(zip(pairs, motions)):
        a, b, v = int(a), int(b), [int(c) for c in v]
        for k in (a, b):
            if k not in bodies:
                bodies[k] = contactsmodel.body(models, instances[k])
        key = (a, b, tuple(v))  # (a pair's answer depends on its instances, their models and its motion alone)
        if key not in seen:
            steps = sweepmodel.path(v)
            hit = -1
            if pair_jobs(instances[a], instances[b], v):  # (without jobs the header says -1; asserted against the walk where it is cheap)
                hit = hit_of(bodies[a], [int(c) for c in instances[a]["box_min"]], bodies[b], [int(c) for c in instances[b]["box_min"]], steps)
            elif len(steps) <= 64:
                assert hit_of(bodies[a], [int(c) for c in instances[a]["box_min"]], bodies[b], [int(c) for c in instances[b]["box_min"]], steps) == -1
            seen[key] = (hit, steps)
        hit, steps = seen[key]
        count += pair_jobs(instances[a], instances[b], v)
        r = sweeps[p]
        r["a"], r["b"] = a, b
        s = r["sweep"]
        s["steps"], s["hit"], s["axis"] = len(steps) - 1, hit, -1
        s["free"] = s["at"] = v if hit < 0 else (0, 0, 0)
        if hit > 0:
            s["at"], s["axis"] = steps[hit]
            s["free"] = steps[hit - 1][0]
            s["sign"] = 1 if v[s["axis"]] > 0 else -1
    summary = dict(hits=int((sweeps["sweep"]["hit"] >= 0).sum()), startsSolid=int((sweeps["sweep"]["hit"] == 0).sum()), jobs=count)
    return sweeps, (contacts_at(models, instances, pairs, sweeps) if want_contacts else None), summary


def contacts_at(models, instances, pairs, sweeps):
    """cvxp_model_contacts' results for the same pairs with instance a of pair p alone replaced by I_a + at_p: one paircontactsmodel.contacts
    per distinct (a, b, at), the pair as given, firstPoint the running sum over the call's pairs."""
    out = np.zeros(len(pairs), dtype=paircontactsmodel.RESULT_DTYPE)
    seen, listed = {}, 0
    for p, (a, b) in enumerate(pairs):
        a, b = int(a), int(b)
        at = tuple(int(c) for c in sweeps["sweep"]["at"][p])
        if (a, b, at) not in seen:
            results, _, _ = paircontactsmodel.contacts(models, [sweepmodel.moved(instances[a], at), instances[b]], [(0, 1)])
            assert (results["overlap"][0] > 0) == (sweeps["sweep"]["hit"][p] >= 0), "the shifted volume is the moved instance's body"
            seen[(a, b, at)] = results[0].copy()
        out[p] = seen[(a, b, at)]
        out[p]["a"], out[p]["b"], out[p]["firstPoint"] = a, b, listed
        listed += int(out[p]["points"])
    return out
