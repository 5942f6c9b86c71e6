"""An independent dense model of cvx_world_spread, written from the contract of include/cpuvox_gpu_spread.h alone.

The world is an (x, y, z) bool volume; the model knows nothing about runs, tiles or 16-bit values.  It is a breadth-first search with a bucket
per start value: the voxels of distance d are settled together, then stepped from.  A large front is handled with numpy, a small one (the single
file of a corridor) cell by cell, so that tens of thousands of levels stay cheap."""
import numpy as np

AIR, SOLID = 0, 1
UNREACHED, BLOCKED = -1, -2
MAX_SEEDS, MAX_STEPS = 4096, 65534
FACES = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))  # bits 0..5 = -X,+X,-Y,+Y,-Z,+Z
_SMALL = 48


def passable(solid, box_min, box_max, medium):
    """Passable(v) over the box as a bool array of shape (X, Z, Y): in the world on all three axes and of the medium."""
    size = [box_max[a] - box_min[a] for a in range(3)]
    out = np.zeros((size[0], size[1], size[2]), dtype=bool)  # (x, y, z)
    lo = [max(box_min[a], 0) for a in range(3)]
    hi = [min(box_max[a], solid.shape[a]) for a in range(3)]
    if all(lo[a] < hi[a] for a in range(3)):
        part = solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        out[lo[0] - box_min[0]:hi[0] - box_min[0], lo[1] - box_min[1]:hi[1] - box_min[1], lo[2] - box_min[2]:hi[2] - box_min[2]] = \
            part if medium == SOLID else ~part
    return np.ascontiguousarray(out.transpose(0, 2, 1))


def field(solid, box_min, box_max, seeds, medium, step_faces, max_steps):
    """-> (the field, int32 of shape (X, Z, Y), and {passable, reached, largestDistance, seedsUsed}).  seeds: (x, y, z, start) or (x, y, z) each."""
    ok = passable(solid, box_min, box_max, medium)
    X, Z, Y = ok.shape
    padded = np.zeros((X + 2, Z + 2, Y + 2), dtype=bool)  # a rim nothing steps onto
    padded[1:-1, 1:-1, 1:-1] = ok
    open_np = padded.ravel()
    open_b = open_np.tobytes()
    sx, sz = (Z + 2) * (Y + 2), Y + 2
    step = {0: -sx, 1: sx, 2: -1, 3: 1, 4: -sz, 5: sz}
    steps = [step[f] for f in range(6) if (step_faces >> f) & 1]
    seen = bytearray(open_np.size)
    seen_np = np.frombuffer(seen, dtype=np.uint8)
    dist = np.full(open_np.size, UNREACHED, dtype=np.int32)
    buckets, used = {}, 0
    for x, y, z, start in (tuple(s) if len(s) == 4 else tuple(s) + (0,) for s in seeds):
        b = (x - box_min[0], y - box_min[1], z - box_min[2])
        if 0 <= b[0] < X and 0 <= b[1] < Y and 0 <= b[2] < Z and ok[b[0], b[2], b[1]]:
            used += 1
            buckets.setdefault(int(start), []).append((b[0] + 1) * sx + (b[2] + 1) * sz + b[1] + 1)
    front, level = [], 0
    while True:
        if len(front) == 0:
            if not buckets:
                break
            level = min(buckets)
        if level > max_steps:
            break
        arriving = buckets.pop(level, [])
        if len(front) + len(arriving) < _SMALL:
            settled = []
            for i in list(front) + arriving:
                if not seen[i]:
                    seen[i] = 1
                    dist[i] = level
                    settled.append(i)
            front = [i + s for i in settled for s in steps if open_b[i + s] and not seen[i + s]]
        else:
            a = np.unique(np.concatenate([np.asarray(front, dtype=np.int64), np.asarray(arriving, dtype=np.int64)]))
            a = a[seen_np[a] == 0]
            seen_np[a] = 1
            dist[a] = level
            n = np.concatenate([a + s for s in steps])
            n = n[open_np[n] & (seen_np[n] == 0)]
            front = n if n.size >= _SMALL else n.tolist()
        level += 1
    out = dist.reshape(X + 2, Z + 2, Y + 2)[1:-1, 1:-1, 1:-1].copy()
    out[~ok] = BLOCKED
    reached = out >= 0
    summary = {"passable": int(ok.sum()), "reached": int(reached.sum()), "largestDistance": int(out.max()) if reached.any() else -1, "seedsUsed": used}
    return out, summary


def slow_field(solid, box_min, box_max, seeds, medium, step_faces, max_steps):
    """The same by plain relaxation until nothing changes (small boxes only): the check of `field`."""
    ok = passable(solid, box_min, box_max, medium)
    X, Z, Y = ok.shape
    big = 1 << 40
    d = np.full((X, Z, Y), big, dtype=np.int64)
    for x, y, z, start in (tuple(s) if len(s) == 4 else tuple(s) + (0,) for s in seeds):
        b = (x - box_min[0], y - box_min[1], z - box_min[2])
        if 0 <= b[0] < X and 0 <= b[1] < Y and 0 <= b[2] < Z and ok[b[0], b[2], b[1]]:
            d[b[0], b[2], b[1]] = min(d[b[0], b[2], b[1]], start)
    while True:
        new = d.copy()
        for f, (dx, dy, dz) in enumerate(FACES):
            if (step_faces >> f) & 1:
                moved = np.full_like(d, big)  # moved[v] = d[v - dir]
                src = d[max(-dx, 0):X - max(dx, 0), max(-dz, 0):Z - max(dz, 0), max(-dy, 0):Y - max(dy, 0)]
                moved[max(dx, 0):X - max(-dx, 0), max(dz, 0):Z - max(-dz, 0), max(dy, 0):Y - max(-dy, 0)] = src
                new = np.minimum(new, moved + 1)
        new[~ok] = big
        if (new == d).all():
            break
        d = new
    out = np.where(d <= max_steps, d, UNREACHED).astype(np.int32)
    out[~ok] = BLOCKED
    return out
