"""cvx_world_brush and cvx_world_pick on the procedural world of bench.py.
Usage: python tools/brush_bench.py [dim] [repeats] [all|old] ; prints one JSON line per measurement.  `old` leaves out the capsule and ellipsoid
cases, so that the script can time the library of an earlier revision beside this one (CVX_GPU_LIB, tools/build_at.sh).

- brush: one FILL sphere of radius 8 / 32 / 128 (LOD 0 + the LOD 1..5 refresh over its footprint) at `repeats` places on the terrain surface:
  device_ms = the call's own stream time (count kernel .. last level patched), call_ms = its wall time; then 64 strokes of radius 8 in one call
  against the same 64 strokes in 64 calls.
- scattered: 64 and 4096 PAINT spheres of radius 8 on the surface all over the world in one call, and the floor of that call: the same rectangle
  (the first two strokes sit in opposite corners) with those two strokes alone.  PAINT, so that every repeat sees the same columns.
- shapes: one PAINT capsule of radius 4 along a space diagonal (10 / 74 / 592 voxels per axis: length 17 / 128 / 1025) and one ellipsoid (64, 16, 64),
  each beside a sphere with the same XZ footprint at the same place; the long capsule as a CARVE beside the route without it: a torch mask of its
  bounding box, built on the device, through cvx_world_write_voxels_device (wall time, mask construction included).
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
new_shapes = (sys.argv[3] if len(sys.argv) > 3 else "all") == "all"
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

# many strokes scattered over the whole world in one call, and the floor of such a call
def scattered(n):
    c = surface(n + 8)[:n]
    c[0], c[1] = (64, c[0][1], 64), (dim - 65, c[1][1], dim - 65)  # (the same rectangle whatever n is)
    return [dict(sphere(v, 8, 0xFF000000 | k), op=gpu.BRUSH_PAINT) for k, v in enumerate(c)]


def median_ms(make, label, **extra):
    dev, wall = [], []
    for _ in range(repeats):
        ms, w = timed(make())
        dev.append(ms)
        wall.append(w)
    out = {"brush": label, "device_ms_median": round(float(np.median(dev)), 3), "device_ms_min": round(min(dev), 3), "device_ms_max": round(max(dev), 3),
           "call_ms_median": round(float(np.median(wall)), 3), "repeats": repeats}
    out.update(extra)
    print(json.dumps(out), flush=True)
    return float(np.median(dev))


floor = median_ms(lambda: scattered(2), "2 spheres r=8 in opposite corners (the rectangle's floor)")
for n in (64, 4096):
    ms = median_ms(lambda: scattered(n), f"{n} spheres r=8 scattered, one call")
    print(json.dumps({"brush": f"{n} scattered / floor", "ratio": round(ms / floor, 2)}), flush=True)

if new_shapes:
    def capsule(a, k, r, op=gpu.BRUSH_PAINT):
        return {"op": op, "shape": gpu.SHAPE_CAPSULE, "a": [int(v) for v in a], "b": [int(a[0]) + k, int(a[1]) - k, int(a[2]) + k], "radius": r, "argb": 0xFF20C040}

    spots = iter(surface(64))
    for k in (10, 74, 592):  # per axis along (1, -1, 1): footprint k + 9 columns, as a sphere of radius (k + 8) / 2 around the middle
        a = next(v for v in spots if v[0] + k + 64 < dim and v[2] + k + 64 < dim)
        mid = [int(a[0]) + k // 2, int(a[1]) - k // 2, int(a[2]) + k // 2]
        c_ms = median_ms(lambda: [capsule(a, k, 4)], f"capsule r=4, {k} per axis")
        s_ms = median_ms(lambda: [dict(sphere(mid, (k + 8) // 2), op=gpu.BRUSH_PAINT)], f"sphere r={(k + 8) // 2}, the same footprint")
        print(json.dumps({"brush": f"capsule {k} per axis / sphere of its footprint", "ratio": round(c_ms / s_ms, 2)}), flush=True)
    a = next(v for v in spots if 80 < v[0] < dim - 80 and 80 < v[2] < dim - 80)
    e_ms = median_ms(lambda: [{"op": gpu.BRUSH_PAINT, "shape": gpu.SHAPE_ELLIPSOID, "a": [int(v) for v in a], "b": [64, 16, 64], "argb": 0xFF20C040}], "ellipsoid (64, 16, 64)")
    s_ms = median_ms(lambda: [dict(sphere(a, 64), op=gpu.BRUSH_PAINT)], "sphere r=64, the same footprint")
    print(json.dumps({"brush": "ellipsoid (64, 16, 64) / sphere of its footprint", "ratio": round(e_ms / s_ms, 2)}), flush=True)

    # the long capsule as a CARVE, and the same tunnel through a dense mask of its bounding box built with torch on the device
    k, r = 592, 4
    a = next(v for v in spots if v[0] + k + 64 < dim and v[2] + k + 64 < dim)
    stroke = capsule(a, k, r, gpu.BRUSH_CARVE)
    A, B = np.array(stroke["a"], dtype=np.int64), np.array(stroke["b"], dtype=np.int64)
    lo, hi = np.minimum(A, B) - r, np.maximum(A, B) + r + 1

    def mask_route():
        torch.cuda.synchronize()
        t = time.perf_counter()
        d = [int(v) for v in B - A]
        L = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        wx = (torch.arange(int(lo[0]), int(hi[0]), device="cuda") - int(A[0])).view(-1, 1, 1)  # (X, Z, Y), y fastest
        wz = (torch.arange(int(lo[2]), int(hi[2]), device="cuda") - int(A[2])).view(1, -1, 1)
        wy = (torch.arange(int(lo[1]), int(hi[1]), device="cuda") - int(A[1])).view(1, 1, -1)
        p = wx * d[0] + wy * d[1] + wz * d[2]
        ww = wx * wx + wy * wy + wz * wz
        mask = torch.where(p <= 0, ww <= r * r, torch.where(p >= L, ww - 2 * p + L <= r * r, ww * L - p * p <= r * r * L)).to(torch.uint8).contiguous()
        torch.cuda.synchronize()
        built = (time.perf_counter() - t) * 1e3
        ms = ctx.write_voxels_device(lo, hi, 0, mask.data_ptr(), gpu.BRUSH_CARVE, 5)
        return built, ms, (time.perf_counter() - t) * 1e3, int(mask.sum().item())

    mask_route()  # (warm-up: torch's kernels and allocations)
    built, ms, wall, voxels = mask_route()
    _, before = ctx.read_voxels(lo, hi, want_argb=False)
    c_dev, c_wall = timed([stroke])
    _, after = ctx.read_voxels(lo, hi, want_argb=False)
    assert (before == after).all(), "the capsule and its dense mask carve different voxels"
    print(json.dumps({"brush": f"CARVE capsule r=4, {k} per axis", "device_ms": round(c_dev, 3), "call_ms": round(c_wall, 3),
                      "mask_route": {"box": [int(v) for v in hi - lo], "mask_voxels": voxels, "mask_build_ms": round(built, 3), "write_device_ms": round(ms, 3),
                                     "total_ms": round(wall, 3)}, "ratio_mask_over_capsule": round(wall / c_wall, 1)}), flush=True)

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
