"""cvx_world_stamp_mesh: mill.obj (tests/golden/mill.obj.xz) stamped on the device.
Usage: python tools/stamp_bench.py [repeats] ; prints one JSON line per measurement.

For mill.obj rescaled to 512, 1024 and 2048 (X flipped, as host.WorldSet.from_obj does):
- empty: into an empty world of the dimensions the rescale asks for, with the LOD 1..5 refresh (device_ms = the call's own stream time, the
  mesh upload .. the last level patched; call_ms = its wall time; the best of `repeats` fresh contexts);
- procedural: into bench.py's 2048^3 procedural world, the model moved by an offset into the middle of it (the best of `repeats` calls on one
  context, so later calls stamp over earlier ones).
host_s: host.WorldSet.from_obj of the same file and size (import, voxeliser, LOD 0 and five downsamples: a different amount of work)."""
import json
import lzma
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
work = tempfile.mkdtemp()
obj = os.path.join(work, "mill.obj")
with lzma.open(os.path.join(ROOT, "tests", "golden", "mill.obj.xz")) as src, open(obj, "wb") as dst:
    dst.write(src.read())


def empty(dims):
    e = np.zeros(0, dtype=np.int32)
    return host.WorldSet.from_voxels(dims, e, e, e, np.zeros(0, dtype=np.uint32))


big = host.WorldSet.procedural(2048, 2048, 2048)
for size in (512, 1024, 2048):
    mesh = host.Mesh.from_obj(obj)
    dims = mesh.rescale(size)
    t0 = time.perf_counter()
    ref = host.WorldSet.from_obj(obj, size)
    host_s = time.perf_counter() - t0
    best = None
    for _ in range(repeats):
        ctx = gpu.Context(0)
        ctx.upload_world(empty(dims))
        ctx.synchronize()
        t0 = time.perf_counter()
        ms = ctx.stamp_mesh(mesh, gpu.BRUSH_FILL, 5)
        call = (time.perf_counter() - t0) * 1e3
        ctx.close()
        best = (ms, call) if best is None or ms < best[0] else best
    print(json.dumps({"stamp": "mill.obj", "into": "empty", "size": size, "dims": list(dims), "lod0_voxels": ref.lod0_voxels,
                      "device_ms": round(best[0], 3), "call_ms": round(best[1], 3), "host_s": round(host_s, 3)}), flush=True)
    # the same model placed into the middle of the procedural world
    v = mesh.vertices
    offset = np.float32([(2048 - dims[0]) // 2, max(0, 2048 - dims[1]) // 2, (2048 - dims[2]) // 2])
    v["position"] += offset
    ctx = gpu.Context(0)
    ctx.upload_world(big)
    ctx.synchronize()
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        ms = ctx.stamp_mesh(mesh, gpu.BRUSH_FILL, 5)
        call = (time.perf_counter() - t0) * 1e3
        best = (ms, call) if best is None or ms < best[0] else best
    ctx.close()
    print(json.dumps({"stamp": "mill.obj", "into": "proc2048", "size": size, "offset": offset.tolist(), "device_ms": round(best[0], 3),
                      "call_ms": round(best[1], 3)}), flush=True)
