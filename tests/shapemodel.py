"""A model of cvx_world_brush's shapes that knows no spans: every stroke's predicate (include/cpuvox_gpu.h) evaluated voxel by voxel.

- apply_strokes: on the dense coordinate grid in int64, folding FILL / CARVE / PAINT in order over (solid, colour).  Boxes and spheres
  included, so that mixed lists work.
- inside: the same predicates with Python integers at given voxels, for strokes at the limits where no dense grid is possible.
Strokes are dicts as cpuvox_amd.gpu.strokes_array takes them, or records of a STROKE_DTYPE array."""
import numpy as np

FILL, CARVE, PAINT = 0, 1, 2
BOX, SPHERE, CAPSULE, ELLIPSOID = 0, 1, 16, 17


def _fields(s):
    """(op, shape, a, b, radius, argb) as Python integers."""
    shape = int(s["shape"])
    a = [int(v) for v in s["a"]]
    names = s.dtype.names if isinstance(s, np.void) else s
    if "b" in names:
        b = s["b"]
        b = [int(b), 0, 0] if np.isscalar(b) else [int(v) for v in b]
    else:
        b = [int(s["radius"]), 0, 0]
    if shape == CAPSULE:
        radius = int(s["pad_"]) if "pad_" in names else int(s["radius"])
    else:
        radius = b[0]
    return int(s["op"]), shape, a, b, radius, int(s["argb"] if "argb" in names else 0) & 0xFFFFFFFF


def _predicate(shape, a, b, r, x, y, z):
    """x, y, z: int64 arrays or Python integers; the arithmetic is the same text for both."""
    if shape == BOX:
        return (x >= a[0]) & (x < b[0]) & (y >= a[1]) & (y < b[1]) & (z >= a[2]) & (z < b[2])
    wx, wy, wz = x - a[0], y - a[1], z - a[2]
    if shape == SPHERE:
        return wx * wx + wy * wy + wz * wz <= r * r
    if shape == ELLIPSOID:
        xx, yy, zz = b[0] * b[0], b[1] * b[1], b[2] * b[2]
        return wx * wx * (yy * zz) + wy * wy * (xx * zz) + wz * wz * (xx * yy) <= xx * yy * zz
    assert shape == CAPSULE, shape
    d = [b[i] - a[i] for i in range(3)]
    L = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    p = wx * d[0] + wy * d[1] + wz * d[2]
    ww = wx * wx + wy * wy + wz * wz
    near_a = ww <= r * r
    if L == 0:
        return near_a
    ux, uy, uz = x - b[0], y - b[1], z - b[2]
    near_b = ux * ux + uy * uy + uz * uz <= r * r
    middle = ww * L - p * p <= r * r * L
    if isinstance(p, np.ndarray):
        return np.where(p <= 0, near_a, np.where(p >= L, near_b, middle))
    return bool(near_a if p <= 0 else (near_b if p >= L else middle))


def stroke_mask(s, dims):
    """The voxels of a (dx, dy, dz) grid inside the stroke: int64 on the dense grid, clipped to the stroke's footprint box first (the products
    are only formed there, which also keeps them in int64 for a stroke far outside the grid)."""
    _, shape, a, b, r, _ = _fields(s)
    lo, hi = [], []
    for i in range(3):
        if shape == BOX:
            l, h = a[i], b[i]
        elif shape == CAPSULE:
            l, h = min(a[i], b[i]) - r, max(a[i], b[i]) + r + 1
        elif shape == ELLIPSOID:
            l, h = a[i] - b[i], a[i] + b[i] + 1
        else:
            l, h = a[i] - r, a[i] + r + 1
        lo.append(max(l, 0))
        hi.append(min(h, dims[i]))
    mask = np.zeros(dims, dtype=bool)
    if any(l >= h for l, h in zip(lo, hi)):
        return mask
    x, y, z = np.meshgrid(*[np.arange(l, h, dtype=np.int64) for l, h in zip(lo, hi)], indexing="ij")
    mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = _predicate(shape, a, b, r, x, y, z)
    return mask


def apply_strokes(solid, colour, strokes):
    """In place: FILL -> solid with argb, CARVE -> air, PAINT -> argb on the solid voxels only; the colour of air is 0."""
    for s in strokes:
        op, _, _, _, _, argb = _fields(s)
        m = stroke_mask(s, solid.shape)
        if op == FILL:
            solid |= m
            colour[m] = np.uint32(argb)
        elif op == CARVE:
            solid &= ~m
        else:
            colour[m & solid] = np.uint32(argb)
    colour[~solid] = 0


def inside(s, x, y, z):
    """The predicate with Python integers at one voxel (any magnitude)."""
    _, shape, a, b, r, _ = _fields(s)
    return bool(_predicate(shape, a, b, r, int(x), int(y), int(z)))
