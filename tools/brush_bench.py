"""cvx_world_brush and cvx_world_pick on the procedural world of bench.py.
Usage: python tools/brush_bench.py [dim] [repeats] ; prints one JSON line per measurement.

- brush: one FILL sphere of radius 8 / 32 / 128 (LOD 0 + the LOD 1..5 refresh over its footprint) at `repeats` places on the terrain surface:
  device_ms = the call's own stream time (count kernel .. last level patched), call_ms = its wall time; then 64 strokes of radius 8 in one call
  against the same 64 strokes in 64 calls.
- pick: the wall time of a call with ONE ray (launch + two copies), and the throughput of 2^20 random rays in one call (wall time of the call,
  copies included, and the kernel alone through cvx_world_pick_device on arrays already on the device)."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays for cvx_world_pick_device; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
build_s = time.perf_counter() - t0
ctx = gpu.Context(0)
ctx.upload_world(ws)
rng = np.random.default_rng(3)


def surface(n):
    """n points on the terrain surface (the first hit of vertical rays at random columns)."""
    xz = rng.integers(64, dim - 64, size=(n, 2))
    o = np.stack([xz[:, 0] + 0.5, np.full(n, dim - 0.5), xz[:, 1] + 0.5], axis=1)
    vox, face, _, _ = ctx.pick(o, np.tile([0.0, -1.0, 0.0], (n, 1)), float(dim))
    return vox[face >= 0]


def sphere(c, r, argb=0xFF3070C0):
    return {"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_SPHERE, "a": [int(v) for v in c], "radius": r, "argb": argb}


def timed(strokes):
    t = time.perf_counter()
    ms = ctx.brush(strokes, 5)
    return ms, (time.perf_counter() - t) * 1e3


timed([sphere(surface(1)[0], 8)])  # (warm-up: the first brush lays the arena out with headroom)
for r in (8, 32, 128):
    dev, wall = [], []
    for c in surface(repeats + 1)[: repeats + 1]:
        ms, w = timed([sphere(c, r)])
        dev.append(ms)
        wall.append(w)
    dev, wall = dev[1:], wall[1:]
    print(json.dumps({"brush": f"sphere r={r}", "levels": "0..5", "device_ms_median": round(float(np.median(dev)), 3), "device_ms_max": round(max(dev), 3),
                      "call_ms_median": round(float(np.median(wall)), 3), "repeats": len(dev)}), flush=True)

centres = surface(64)
strokes = [sphere(c, 8, 0xFF000000 | k) for k, c in enumerate(centres)]
one_dev, one_wall = timed(strokes)
many_dev, many_wall = 0.0, 0.0
for s in strokes:
    ms, w = timed([s])
    many_dev += ms
    many_wall += w
print(json.dumps({"brush": f"{len(strokes)} spheres r=8", "one_call_device_ms": round(one_dev, 3), "one_call_ms": round(one_wall, 3),
                  "separate_calls_device_ms": round(many_dev, 3), "separate_calls_ms": round(many_wall, 3)}), flush=True)
used, abandoned, spare = ctx.edit_stats()

# pick latency: one ray per call
o1, d1 = np.float32([[dim / 2, dim - 1.0, dim / 2]]), np.float32([[0.3, -1.0, 0.2]])
for _ in range(10):
    ctx.pick(o1, d1, 1e9)
lat = []
for _ in range(200):
    t = time.perf_counter()
    ctx.pick(o1, d1, 1e9)
    lat.append((time.perf_counter() - t) * 1e6)
print(json.dumps({"pick": "1 ray", "call_us_median": round(float(np.median(lat)), 1), "call_us_p95": round(float(np.percentile(lat, 95)), 1)}), flush=True)

# pick throughput: 2^20 random rays from random points towards random points of the world
n = 1 << 20
o = (rng.uniform(0.0, 1.0, size=(n, 3)) * dim).astype(np.float32)
o[:, 1] = rng.uniform(0.3, 1.0, size=n) * dim
d = (rng.uniform(0.0, 1.0, size=(n, 3)) * dim - o).astype(np.float32)
ctx.pick(o, d, 1e9)
walls = []
for _ in range(5):
    t = time.perf_counter()
    vox, face, _, _ = ctx.pick(o, d, 1e9)
    walls.append(time.perf_counter() - t)
rays = np.zeros(n, dtype=gpu.PICK_RAY_DTYPE)
rays["origin"], rays["direction"], rays["maxT"] = o, d, 1e9
dr = torch.from_numpy(rays.view(np.uint8)).cuda()
dh = torch.empty(n * gpu.PICK_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
side = torch.cuda.Stream()  # (a stream of its own: torch's default stream has the handle 0, which cvx_world_pick_device reads as "the context's")
lib = gpu.lib()
torch.cuda.synchronize()
kern = []
with torch.cuda.stream(side):
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        assert lib.cvx_world_pick_device(ctx._h, n, C.c_void_p(dr.data_ptr()), C.c_void_p(dh.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
        b.record(side)
        side.synchronize()
        kern.append(a.elapsed_time(b))
kern = kern[1:]
same = np.frombuffer(dh.cpu().numpy().tobytes(), dtype=gpu.PICK_HIT_DTYPE)
assert (same["voxel"] == vox).all() and (same["face"] == face).all(), "cvx_world_pick_device and cvx_world_pick disagree"
print(json.dumps({"pick": f"{n} random rays", "hit_fraction": round(float((face >= 0).mean()), 3),
                  "call_ms_median": round(float(np.median(walls)) * 1e3, 3), "call_Mrays_per_s": round(n / float(np.median(walls)) / 1e6, 1),
                  "kernel_ms_median": round(float(np.median(kern)), 3), "kernel_Mrays_per_s": round(n / float(np.median(kern)) / 1e3, 1)}), flush=True)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(build_s, 1), "arena_used_MB": round(used / 1e6, 1), "abandoned_MB": round(abandoned / 1e6, 2),
                  "spare_MB": round(spare / 1e6, 1)}), flush=True)
ctx.close()
