"""cvx_world_copy on the procedural world of bench.py.
Usage: python tools/copy_bench.py [dim] [repeats] ; prints one JSON line per measurement.

Every call refreshes LOD 1..5 over its rectangle; device_ms = the call's own stream time (count kernel .. last level patched), call_ms = its wall
time.  Boxes sit on the terrain surface (the first hit of a vertical ray), so that they hold terrain and air.
- one 64^3 copy (REPLACE), and a FILL brush box over the same destination for comparison;
- a 256 x 64 x 256 move that overlaps itself (shifted by 64, 0, 32);
- the 16 transforms of one 32^3 box, one call each;
- 512 scattered 16^3 placements in one call, against the same placements in 512 calls."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
build_s = time.perf_counter() - t0
ctx = gpu.Context(0)
ctx.upload_world(ws)
rng = np.random.default_rng(3)


def surface(n, margin=320):
    """n voxels on the terrain surface at random columns at least `margin` away from the world's edges."""
    xz = rng.integers(margin, dim - margin, size=(n, 2))
    o = np.stack([xz[:, 0] + 0.5, np.full(n, dim - 0.5), xz[:, 1] + 0.5], axis=1)
    vox, face, _, _ = ctx.pick(o, np.tile([0.0, -1.0, 0.0], (n, 1)), float(dim))
    return vox[face >= 0]


def box_at(c, size):
    """A box of `size` whose top third is above the surface voxel c: (srcMin, srcMax)."""
    lo = [int(c[0]) - size[0] // 2, max(0, int(c[1]) - 2 * size[1] // 3), int(c[2]) - size[2] // 2]
    return lo, [lo[0] + size[0], lo[1] + size[1], lo[2] + size[2]]


def placement(src, dst, transform=0, op=gpu.COPY_REPLACE, move=0):
    return {"srcMin": src[0], "srcMax": src[1], "dst": dst, "transform": transform, "op": op, "move": move}


def timed(call, arg):
    t = time.perf_counter()
    ms = call(arg, 5)
    return ms, (time.perf_counter() - t) * 1e3


def report(name, samples, **extra):
    dev, wall = [s[0] for s in samples], [s[1] for s in samples]
    print(json.dumps({"copy": name, "levels": "0..5", "device_ms_median": round(float(np.median(dev)), 3), "device_ms_max": round(max(dev), 3),
                      "call_ms_median": round(float(np.median(wall)), 3), "repeats": len(dev), **extra}), flush=True)


ctx.brush([{"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_SPHERE, "a": [int(v) for v in surface(1)[0]], "radius": 4, "argb": 0xFF3070C0}], 5)  # (warm-up)

# one 64^3 copy, and a brush box over the same destination
copies, brushes = [], []
for _ in range(repeats):
    a, b = surface(2)[:2]
    src = box_at(a, (64, 64, 64))
    dst = box_at(b, (64, 64, 64))[0]
    copies.append(timed(ctx.copy, [placement(src, dst)]))
    brushes.append(timed(ctx.brush, [{"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": dst, "b": [dst[i] + 64 for i in range(3)], "argb": 0xFF3070C0}]))
report("one 64^3 box", copies)
report("brush: a 64^3 FILL box over the same destination", brushes)

# a 256 x 64 x 256 move that overlaps itself
moves = []
for _ in range(repeats):
    src = box_at(surface(1)[0], (256, 64, 256))
    moves.append(timed(ctx.copy, [placement(src, [src[0][0] + 64, src[0][1], src[0][2] + 32], move=1)]))
report("256 x 64 x 256 move overlapping itself (shift 64, 0, 32)", moves)

# the 16 transforms of one 32^3 box
c = surface(2)
src = box_at(c[0], (32, 32, 32))
dst = box_at(c[1], (32, 32, 32))[0]
turns = [timed(ctx.copy, [placement(src, dst, t)]) for t in range(16)]
report("32^3 box, each of the 16 transforms", turns, calls=16)

# 512 scattered 16^3 placements: one call against 512 calls
points = surface(1200, margin=64)[:1024]  # (a vertical ray can miss: a column without voxels)
assert len(points) == 1024
scatter = [placement(box_at(points[2 * k], (16, 16, 16)), box_at(points[2 * k + 1], (16, 16, 16))[0], k % 16) for k in range(512)]
one = timed(ctx.copy, scatter)
many_dev = many_wall = 0.0
for p in scatter:
    ms, w = timed(ctx.copy, [p])
    many_dev += ms
    many_wall += w
print(json.dumps({"copy": f"{len(scatter)} scattered 16^3 boxes", "one_call_device_ms": round(one[0], 3), "one_call_ms": round(one[1], 3),
                  "separate_calls_device_ms": round(many_dev, 3), "separate_calls_ms": round(many_wall, 3)}), flush=True)
used, abandoned, spare = ctx.edit_stats()
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(build_s, 1), "arena_used_MB": round(used / 1e6, 1), "abandoned_MB": round(abandoned / 1e6, 2),
                  "spare_MB": round(spare / 1e6, 1)}), flush=True)
ctx.close()
