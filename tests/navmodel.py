"""The dense model of cvx_world_nav_build / cvx_nav_query (include/cpuvox_gpu.h): straight from the voxel rule, independent of the interval
form the library computes.  B is the OR of the shifted numpy volume, stand cells and steps come from clear ranges (cumulative sums of B along
y), distances from scipy's Dijkstra on the reversed step graph, `next` from the stated order.

analyse(solid, box_min, box_max, width, height, step_up, max_drop, goals, max_steps) -> (steps, summary): steps[x, y, z] is the cvx_nav_step
the query of position (x, y, z) must give, for every voxel of the world; summary holds the deterministic fields of cvx_nav_summary."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

STEP_DTYPE = np.dtype([("cell", "<i4", 3), ("distance", "<i4"), ("next", "<i4", 3), ("direction", "<i4")])  # cvx_nav_step
SUMMARY_NAMES = ("nodes", "reached", "goalsResolved", "largestDistance", "columnsWithSeveralNodes")
DIRECTIONS = ((-1, 0, 0), (1, 0, 1), (0, -1, 4), (0, 1, 5))  # (dx, dz, the pick's face number), in the order of the next choice


def clip_box(dims, box_min, box_max):
    lo = [max(0, int(box_min[a])) for a in range(3)]
    hi = [min(int(dims[a]), int(box_max[a])) for a in range(3)]
    return None if any(lo[a] >= hi[a] for a in range(3)) else (lo, hi)


def blocked(solid, width, pad):
    """B[x, y, z] for 0 <= x <= dimX - width, 0 <= z <= dimZ - width and 0 <= y < dimY + pad (air above the world)."""
    dx, dy, dz = solid.shape
    out = np.zeros((dx - width + 1, dy + pad, dz - width + 1), dtype=bool)
    for i in range(width):
        for k in range(width):
            out[:, :dy, :] |= solid[i:i + dx - width + 1, :, k:k + dz - width + 1]
    return out


def stand_cells(solid, width, height):
    """The stand cells of the whole world for a width x height x width body, as an (n, 3) array in (x, y, z) order (the tests pick goals here)."""
    B = blocked(solid, width, height + 1)
    dy = solid.shape[1]
    stand = np.ones(B.shape, dtype=bool)
    stand[:, 1:, :] = B[:, :-1, :]
    for j in range(height):
        stand[:, :B.shape[1] - j, :] &= ~B[:, j:, :]
    stand[:, dy:, :] = False
    return np.argwhere(stand)


def analyse(solid, box_min, box_max, width, height, step_up, max_drop, goals, max_steps=0):
    dims = solid.shape
    dx, dy, dz = dims
    steps = np.zeros(dims, dtype=STEP_DTYPE)
    for name in ("cell", "distance", "next", "direction"):
        steps[name] = -1
    summary = dict.fromkeys(SUMMARY_NAMES, 0)
    box = clip_box(dims, box_min, box_max)
    assert box is not None
    (x0, y0, z0), (x1, y1, z1) = box
    if x1 - x0 < width or z1 - z0 < width:
        return steps, summary
    pad = height + step_up + 1
    B = blocked(solid, width, pad)
    cs = np.zeros((B.shape[0], B.shape[1] + 1, B.shape[2]), dtype=np.int32)  # cs[:, b] - cs[:, a] = blocked voxels of y in [a, b)
    np.cumsum(B, axis=1, out=cs[:, 1:, :])
    in_grid = np.zeros(B.shape, dtype=bool)
    in_grid[x0:x1 - width + 1, y0:y1, z0:z1 - width + 1] = True
    floor_below = np.ones(B.shape, dtype=bool)
    floor_below[:, 1:, :] = B[:, :-1, :]
    top = B.shape[1]
    clear_h = np.zeros(B.shape, dtype=bool)
    clear_h[:, :top - height + 1, :] = (cs[:, height:, :] - cs[:, :top - height + 1, :]) == 0
    stand = in_grid & clear_h & floor_below
    sx, sy, sz = np.nonzero(stand)
    n = len(sx)
    node = np.full(B.shape, -1, dtype=np.int64)
    node[sx, sy, sz] = np.arange(n)
    summary["nodes"] = n
    per_column = stand.sum(axis=1)
    summary["columnsWithSeveralNodes"] = int((per_column >= 2).sum())

    def clear(x, a, b, z):  # B false for a <= y < b
        return cs[x, b, z] == cs[x, a, z]

    src, dst, way = [], [], []
    for k, (ddx, ddz, _) in enumerate(DIRECTIONS):
        bx, bz = sx + ddx, sz + ddz
        inside = (bx >= 0) & (bx < B.shape[0]) & (bz >= 0) & (bz < B.shape[2])
        for d in range(-min(max_drop, dy), step_up + 1):
            by = sy + d
            ok = inside & (by >= 0) & (by < dy)
            a = np.nonzero(ok)[0]
            b = node[bx[a], by[a], bz[a]]
            keep = b >= 0
            a, b = a[keep], b[keep]
            t = np.maximum(sy[a], sy[b]) + height
            keep = clear(sx[a], sy[a], t, sz[a]) & clear(sx[b], sy[b], t, sz[b])
            src.append(a[keep])
            dst.append(b[keep])
            way.append(np.full(int(keep.sum()), k))
    src, dst, way = (np.concatenate(v) if v else np.zeros(0, dtype=np.int64) for v in (src, dst, way))

    # where a position falls to: the lowest y' with B false for y' .. y, for every (x, y, z) of the padded grid
    fall = np.full(B.shape, -1, dtype=np.int64)
    for y in range(B.shape[1]):
        free = ~B[:, y, :]
        if y == 0:
            fall[:, 0, :] = np.where(free, 0, -1)
        else:
            fall[:, y, :] = np.where(free, np.where(B[:, y - 1, :], y, fall[:, y - 1, :]), -1)

    def resolve(px, py, pz):
        if not (x0 <= px <= x1 - width and z0 <= pz <= z1 - width) or py < 0:
            return -1
        y = int(fall[px, min(py, dy), pz])
        return int(node[px, y, pz]) if y >= 0 else -1

    goal_nodes = [resolve(*[int(v) for v in g]) for g in np.asarray(goals, dtype=np.int64).reshape(-1, 3)]
    summary["goalsResolved"] = sum(1 for g in goal_nodes if g >= 0)
    dist = np.full(n, np.inf)
    sources = sorted({g for g in goal_nodes if g >= 0})
    if sources and n:
        reverse = csr_matrix((np.ones(len(src)), (dst, src)), shape=(n, n))
        dist = dijkstra(reverse, directed=True, indices=sources, unweighted=True, min_only=True, limit=float(max_steps) if max_steps > 0 else np.inf)
    reached = np.isfinite(dist)
    d = np.where(reached, dist, -1).astype(np.int64)
    summary["reached"] = int(reached.sum())
    summary["largestDistance"] = int(d.max()) if reached.any() else 0

    # next: among the steps to distance - 1 the first direction, in it the highest target
    nxt = np.full((n, 3), -1, dtype=np.int64)
    direction = np.full(n, -1, dtype=np.int64)
    at_goal = reached & (d == 0)
    nxt[at_goal] = np.stack([sx, sy, sz], axis=1)[at_goal]
    good = reached[src] & reached[dst] & (d[src] > 0) & (d[dst] == d[src] - 1)
    es, ed, ew = src[good], dst[good], way[good]
    order = np.lexsort((-sy[ed], ew, es))
    es, ed, ew = es[order], ed[order], ew[order]
    first = np.ones(len(es), dtype=bool)
    first[1:] = es[1:] != es[:-1]
    es, ed, ew = es[first], ed[first], ew[first]
    nxt[es] = np.stack([sx[ed], sy[ed], sz[ed]], axis=1)
    direction[es] = np.array([f for _, _, f in DIRECTIONS])[ew]
    assert (reached & (d > 0) & (direction < 0)).sum() == 0, "a reached node without a step to distance - 1"

    # the query of every voxel position
    where = np.full(dims, -1, dtype=np.int64)
    gx0, gx1, gz0, gz1 = x0, x1 - width + 1, z0, z1 - width + 1
    f = fall[gx0:gx1, :dy, gz0:gz1]
    xs, ys, zs = np.nonzero(f >= 0)
    where[gx0:gx1, :, gz0:gz1][xs, ys, zs] = node[xs + gx0, f[xs, ys, zs], zs + gz0]
    qx, qy, qz = np.nonzero(where >= 0)
    i = where[qx, qy, qz]
    steps["cell"][qx, qy, qz] = np.stack([sx[i], sy[i], sz[i]], axis=1)
    steps["distance"][qx, qy, qz] = d[i]
    steps["next"][qx, qy, qz] = nxt[i]
    steps["direction"][qx, qy, qz] = direction[i]
    return steps, summary


def query(steps, cells):
    """What cvx_nav_query gives for the positions `cells` (int triples).  Beside the world or below y = 0: no cell.  Above the world a position
    lies in its column's topmost air interval, the one (x, dimY - 1, z) lies in unless that voxel is blocked -- and then the interval's floor is
    dimY, outside every box: no cell either way."""
    dx, dy, dz = steps.shape
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(cells), dtype=STEP_DTYPE)
    for name in ("cell", "distance", "next", "direction"):
        out[name] = -1
    for k, (x, y, z) in enumerate(cells):
        if 0 <= x < dx and 0 <= z < dz and y >= 0:
            out[k] = steps[x, min(y, dy - 1), z]
    return out
