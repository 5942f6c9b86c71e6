"""Dense numpy model of cvx_world_move, written from the contract in include/cpuvox_gpu.h; it shares no code with cpuvox_amd/csrc/cvx_move.h.

The world is a boolean volume solid[x, y, z]; Volume.box() cuts any box of voxels out of the volume padded per the body's flags (or tiled, for a
repeating world).  A leg is tested the slow way: the box is pushed along its axis to every offset at which it starts to cover a new slab of voxels,
and it stops one unit before the first offset at which it overlaps a solid voxel it did not overlap when the leg started.

move(solid, body, repeat) -> (pos, flags); overlaps(solid, pos, size, flags, repeat) is the invariant's test."""
import numpy as np

UNIT = 256
SOLID_BELOW, SOLID_SIDES = 1, 2
RESTING, STARTS_SOLID, STEPPED, INVALID = 1 << 6, 1 << 7, 1 << 8, -(1 << 31)
BLOCKED = {(0, -1): 1, (0, 1): 2, (1, -1): 4, (1, 1): 8, (2, -1): 16, (2, 1): 32}
MAX_SIZE, MAX_DELTA, MAX_STEP_UP, MAX_POS = 64 * UNIT, 256 * UNIT, 4 * UNIT, 1 << 28


def body(pos, size, delta=(0, 0, 0), step_up=0, flags=0):
    return {"pos": [int(v) for v in pos], "size": [int(v) for v in size], "delta": [int(v) for v in delta], "stepUp": int(step_up), "flags": int(flags)}


def valid(b):
    return (all(1 <= s <= MAX_SIZE for s in b["size"]) and all(abs(d) <= MAX_DELTA for d in b["delta"]) and all(abs(p) <= MAX_POS for p in b["pos"])
            and 0 <= b["stepUp"] <= MAX_STEP_UP and 0 <= b["flags"] <= 3)


class Volume:
    def __init__(self, solid, flags, repeat):
        self.solid, self.repeat = solid, bool(repeat)
        self.below, self.sides = bool(flags & SOLID_BELOW), bool(flags & SOLID_SIDES) and not repeat

    def box(self, lo, hi):
        """solid voxels of the padded volume in lo[a] .. hi[a] (inclusive, any integers) as a dense array"""
        gx, gy, gz = self.solid.shape
        xs, ys, zs = (np.arange(lo[a], hi[a] + 1) for a in range(3))
        if self.repeat:
            inside = np.ones((len(xs), len(zs)), dtype=bool)
            xi, zi = xs % gx, zs % gz
        else:
            inside = ((xs >= 0) & (xs < gx))[:, None] & ((zs >= 0) & (zs < gz))[None, :]
            xi, zi = np.clip(xs, 0, gx - 1), np.clip(zs, 0, gz - 1)
        out = self.solid[np.ix_(xi, np.clip(ys, 0, gy - 1), zi)]
        out = np.where(inside[:, None, :], out, self.sides)
        out[:, ys < 0, :] = self.below
        out[:, ys >= gy, :] = False
        return out


def _cover(pos, size):
    return [p // UNIT for p in pos], [(p + s - 1) // UNIT for p, s in zip(pos, size)]


def overlaps(solid, pos, size, flags, repeat):
    return bool(Volume(solid, flags, repeat).box(*_cover(pos, size)).any())


def _leg(vol, pos, size, axis, d):
    """-> (new pos, moved < |d|)"""
    sign = 1 if d > 0 else -1
    lo, hi = _cover(pos, size)
    # the voxels the box sweeps beyond those it covers now, as one box
    far = list(pos)
    far[axis] += d
    flo, fhi = _cover(far, size)
    if sign > 0:
        new_lo, new_hi = hi[axis] + 1, fhi[axis]
    else:
        new_lo, new_hi = flo[axis], lo[axis] - 1
    moved = abs(d)
    if new_lo <= new_hi:
        blo, bhi = list(lo), list(hi)
        blo[axis], bhi[axis] = new_lo, new_hi
        slabs = vol.box(blo, bhi).any(axis=tuple(a for a in range(3) if a != axis))  # per new slab: anything solid in the cross-section
        if slabs.any():
            k = new_lo + int(np.argmax(slabs)) if sign > 0 else new_hi - int(np.argmax(slabs[::-1]))
            # the first offset m at which the box covers slab k; it stops at m - 1
            ms = np.arange(1, abs(d) + 1, dtype=np.int64)  # unit by unit
            covers = (pos[axis] + ms + size[axis] - 1) // UNIT >= k if sign > 0 else (pos[axis] - ms) // UNIT <= k
            moved = int(ms[np.argmax(covers)]) - 1
    out = list(pos)
    out[axis] += sign * moved
    return out, moved < abs(d)


def _resting(vol, pos, size):
    if pos[1] % UNIT:
        return False
    lo, hi = _cover(pos, size)
    k = pos[1] // UNIT - 1
    return bool(vol.box([lo[0], k, lo[2]], [hi[0], k, hi[2]]).any())


def move(solid, b, repeat=False):
    if not valid(b):
        return list(b["pos"]), INVALID
    vol = Volume(solid, b["flags"], repeat)
    p0, size, (dx, dy, dz) = list(b["pos"]), b["size"], b["delta"]
    flags = STARTS_SOLID if vol.box(*_cover(p0, size)).any() else 0
    pos, blocked, down_blocked = p0, 0, False
    for axis, d in ((1, dy), (0, dx), (2, dz)):
        if d:
            pos, hit = _leg(vol, pos, size, axis, d)
            if hit:
                blocked |= BLOCKED[(axis, 1 if d > 0 else -1)]
                down_blocked |= axis == 1 and d < 0
    if b["stepUp"] > 0 and dy <= 0 and blocked & (1 | 2 | 16 | 32) and (down_blocked or (dy == 0 and _resting(vol, p0, size))):
        q, _ = _leg(vol, p0, size, 1, b["stepUp"])
        r = q[1] - p0[1]
        blocked_b = STEPPED
        for axis, d in ((0, dx), (2, dz), (1, -(r - dy))):
            if d:
                q, hit = _leg(vol, q, size, axis, d)
                if hit:
                    blocked_b |= BLOCKED[(axis, 1 if d > 0 else -1)]
        if abs(q[0] - p0[0]) + abs(q[2] - p0[2]) > abs(pos[0] - p0[0]) + abs(pos[2] - p0[2]):
            pos, blocked = q, blocked_b
    flags |= blocked
    if _resting(vol, pos, size):
        flags |= RESTING
    return pos, flags
