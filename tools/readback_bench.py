"""cvx_world_read_level / cvx_world_read_region and cvx_world_compact on the procedural world of bench.py.
Usage: python tools/readback_bench.py [dim] [repeats] ; prints one JSON line per measurement.

- read_level: every level 0..5 (bytes of the blob, wall time of the call: count, scan, write and the device-to-host copy into malloc'd memory).
- read_region: LOD-0 rectangles of 32^2 .. 512^2 columns at `repeats` places (wall time of the call).
- compact: after 64 separate radius-8 brushes, and after 1000 brushes scattered over the world: bytes reclaimed, device_ms = the call's own
  stream time (count kernels .. last move), call_ms = its wall time; then the first brush after the compaction (device and wall time)."""
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


def wall(fn, *args):
    t = time.perf_counter()
    out = fn(*args)
    return out, (time.perf_counter() - t) * 1e3


def surface(n):
    """n points on the terrain surface (the first hit of vertical rays at random columns)."""
    xz = rng.integers(64, dim - 64, size=(n, 2))
    o = np.stack([xz[:, 0] + 0.5, np.full(n, dim - 0.5), xz[:, 1] + 0.5], axis=1)
    vox, face, _, _ = ctx.pick(o, np.tile([0.0, -1.0, 0.0], (n, 1)), float(dim))
    return vox[face >= 0]


def sphere(c, r, argb=0xFF3070C0):
    return {"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_SPHERE, "a": [int(v) for v in c], "radius": r, "argb": argb}


ctx.read_level(5)  # (warm-up: places the levels in the arena)
for lod in range(6):
    (blob, _), _ = wall(ctx.read_level, lod)
    assert blob == ws.storage(lod).tobytes(), f"LOD {lod} is not what was uploaded"
    times = [wall(ctx.read_level, lod)[1] for _ in range(repeats)]
    ms = float(np.median(times))
    print(json.dumps({"read_level": lod, "bytes": len(blob), "call_ms_median": round(ms, 3), "call_ms_max": round(max(times), 3),
                      "GB_per_s": round(len(blob) / ms / 1e6, 2), "repeats": repeats}), flush=True)

for size in (32, 64, 128, 256, 512):
    times, nbytes = [], 0
    for _ in range(repeats + 1):
        x0, z0 = (int(v) for v in rng.integers(0, dim - size, 2))
        (blob, _), ms = wall(ctx.read_region, 0, x0, z0, size, size)
        times.append(ms)
        nbytes = len(blob)
    times = times[1:]
    print(json.dumps({"read_region": f"{size}^2", "bytes": nbytes, "call_ms_median": round(float(np.median(times)), 3),
                      "call_ms_max": round(max(times), 3), "repeats": len(times)}), flush=True)


def compact(label):
    used, abandoned, spare = ctx.edit_stats()
    (reclaimed, dev), call = wall(ctx.compact)
    used2, abandoned2, spare2 = ctx.edit_stats()
    print(json.dumps({"compact": label, "reclaimed_MB": round(reclaimed / 1e6, 3), "abandoned_before_MB": round(abandoned / 1e6, 3),
                      "used_before_MB": round(used / 1e6, 1), "used_after_MB": round(used2 / 1e6, 1), "spare_after_MB": round(spare2 / 1e6, 2),
                      "device_ms": round(dev, 3), "call_ms": round(call, 3)}), flush=True)
    c = surface(1)[0]
    dev_b, call_b = wall(ctx.brush, [sphere(c, 8)], 5)
    print(json.dumps({"first_brush_after_compact": label, "device_ms": round(dev_b, 3), "call_ms": round(call_b, 3)}), flush=True)


for c in surface(64):
    ctx.brush([sphere(c, 8)], 5)
compact("after 64 brushes r=8")
for k, c in enumerate(surface(1200)[:1000]):
    ctx.brush([sphere(c, int(rng.integers(2, 17)), 0xFF000000 | k)], 5)
compact("after 1000 scattered brushes")
(reclaimed, dev), call = wall(ctx.compact)
print(json.dumps({"compact": "again, after one more brush", "reclaimed_MB": round(reclaimed / 1e6, 3), "device_ms": round(dev, 3), "call_ms": round(call, 3)}), flush=True)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(build_s, 1), "level_bytes": [ws.info(k).byteLength for k in range(6)]}), flush=True)
ctx.close()
