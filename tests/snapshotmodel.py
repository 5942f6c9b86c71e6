"""A dense model of cvx_world_snapshot_diff, written from include/cpuvox_gpu_snapshot.h alone: two worlds as (X, Z, Y) arrays, y fastest (what
cvx_world_read_voxels returns), compared voxel by voxel.  Nothing here knows runs, records or blobs."""
import numpy as np

IGNORE_COLOUR = 1
CHANGE_DTYPE = np.dtype([("x", "<i4"), ("z", "<i4"), ("yMin", "<i4"), ("yMax", "<i4")])


def differs(before, after, flags=0):
    """before, after: (solid bool (X, Z, Y), argb uint32 (X, Z, Y)) -> bool (X, Z, Y): solid in one and air in the other, or solid in both with
    different colour words (under IGNORE_COLOUR solidity alone)."""
    (sb, cb), (sa, ca) = before, after
    out = sb != sa
    if not flags & IGNORE_COLOUR:
        out = out | (sb & sa & (cb != ca))
    return out


def diff(before, after, origin=(0, 0), flags=0):
    """-> (the changed columns as a CHANGE_DTYPE array, x ascending then z, yMin the lowest differing y and yMax the highest + 1; the summary:
    changedColumns, changedVoxels, min and max of the differing voxels' box, all 0 when nothing differs).  origin: the (x, z) of element [0, 0]."""
    d = differs(before, after, flags)
    height = d.shape[2]
    xs, zs = np.nonzero(d.any(axis=2))  # (row-major: x ascending, then z)
    changes = np.zeros(len(xs), dtype=CHANGE_DTYPE)
    changes["x"], changes["z"] = xs + origin[0], zs + origin[1]
    changes["yMin"] = d[xs, zs].argmax(axis=1) if len(xs) else 0
    changes["yMax"] = height - d[xs, zs][:, ::-1].argmax(axis=1) if len(xs) else 0
    summary = {"changedColumns": len(xs), "changedVoxels": int(d.sum()), "min": (0, 0, 0), "max": (0, 0, 0)}
    if len(xs):
        summary["min"] = (int(changes["x"].min()), int(changes["yMin"].min()), int(changes["z"].min()))
        summary["max"] = (int(changes["x"].max()) + 1, int(changes["yMax"].max()), int(changes["z"].max()) + 1)
    return changes, summary
