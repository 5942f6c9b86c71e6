"""cvx_world_edit (a LOD-0 rectangle + the device LOD refresh of LOD 1..5 over it) against a full re-upload, on the procedural world of bench.py.
Usage: python tools/edit_bench.py [dim] [repeats] ; prints one JSON line per rectangle size and one for the re-upload.

Each edit replaces a size x size rectangle with the columns of another rectangle of the same world (real terrain, so colour blocks move and run
lists change), at `repeats` places; device_ms is the call's own stream time (sub-blob upload .. last level patched), call_ms the wall time of the
call (host validation included).  The re-upload is cvx_world_upload of all six levels + the arena rebuild the next draw does (the draw's own time
taken out)."""
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
W, H = 1920, 1080
t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
build_s = time.perf_counter() - t0
pose = host.camera_pose(*host.sample_benchmark_path(0.3, ws.dims), W, H)
lods, far = host.setup_lods(pose, ws.max_dimension, W, H, 1.0)
frame = host.setup_frame(pose, lods, far, W, H, ws.dims[1])

ctx = gpu.Context(0)
ctx.upload_world(ws)
ctx.set_resolution(W, H)


def draw_s():
    t = time.perf_counter()
    ctx.draw_segments(frame, 0)
    return time.perf_counter() - t


draw_s()
plain = min(draw_s() for _ in range(5))
rng = np.random.default_rng(1)
results = []
for size in (32, 64, 128, 256, 512):
    if size > dim // 2:
        break
    dev, wall = [], []
    for r in range(repeats + 1):
        x0, z0 = (int(v) * 32 for v in rng.integers(0, (dim - size) // 32, 2))
        sx, sz = (int(v) * 32 for v in rng.integers(0, (dim - size) // 32, 2))
        blob, count = ws.extract_region(0, sx, sz, size, size)
        t = time.perf_counter()
        ms = ctx.edit(x0, z0, size, size, blob, count, 5)
        w = time.perf_counter() - t
        if r:  # (the first call of a size: warm-up; the very first also lays the arena out with headroom)
            dev.append(ms)
            wall.append(w * 1e3)
    used, abandoned, spare = ctx.edit_stats()
    line = {"edit": f"{size}x{size}", "levels": "0..5", "device_ms_median": round(float(np.median(dev)), 3), "device_ms_max": round(max(dev), 3),
            "call_ms_median": round(float(np.median(wall)), 3), "repeats": repeats, "arena_used_MB": round(used / 1e6, 1),
            "abandoned_MB": round(abandoned / 1e6, 2), "spare_MB": round(spare / 1e6, 1)}
    results.append(line)
    print(json.dumps(line), flush=True)

uploads = []
for _ in range(3):
    t = time.perf_counter()
    ctx.upload_world(ws)
    ctx.draw_segments(frame, 0)
    uploads.append((time.perf_counter() - t - plain) * 1e3)
print(json.dumps({"full_reupload_ms_median": round(float(np.median(uploads)), 1), "world": f"proc{dim}", "world_build_s": round(build_s, 1),
                  "arena_MB": round(ctx.edit_stats()[0] / 1e6, 1), "draw_ms": round(plain * 1e3, 3)}), flush=True)
ctx.close()
