"""cvx_world_pieces on mill512 and on the procedural world of bench.py, after one sphere carve.
Usage: python tools/pieces_bench.py [dim] [repeats] ; prints one JSON line per world.

Per world: solid runs (nodes) and pieces, device_ms of a REPORT over the whole world and over a 256^3 box around the carve (median of `repeats`),
the REMOVE (LOD 1..5 refreshed), and beside them the route a host had before this call, timed in the same run: cvx_world_read_level of LOD 0 plus
the sequential union-find of tests/pieces_rules.cpp over the blob (its own milliseconds, without loading the blob).  anchors = GROUND | LARGEST."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import scenes  # noqa: E402
import ruleslib  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
ANCHORS = gpu.ANCHOR_GROUND | gpu.ANCHOR_LARGEST
work = tempfile.mkdtemp(prefix="pieces_bench")
rules = ruleslib.build("pieces_rules", work, "-O2")


def median_ms(call):
    return round(float(np.median([call() for _ in range(repeats)])), 3)


def bench(name, ws):
    dims = tuple(ws.dims)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    # the carve: a sphere around a surface voxel near the middle of the world
    o = np.array([[dims[0] * 0.5 + 0.5, dims[1] - 0.5, dims[2] * 0.5 + 0.5]])
    vox, face, _, _ = ctx.pick(o, np.array([[0.0, -1.0, 0.0]]), float(dims[1]))
    centre = [int(v) for v in vox[0]] if face[0] >= 0 else [dims[0] // 2, dims[1] // 4, dims[2] // 2]
    ctx.brush([{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_SPHERE, "a": centre, "radius": min(48, dims[0] // 8)}], 5)
    whole = ((0, 0, 0), dims)
    near = ([max(0, c - 128) for c in centre], [c + 128 for c in centre])
    _, summary, _ = ctx.world_pieces(*whole, ANCHORS)  # (warm-up)
    whole_ms = median_ms(lambda: ctx.world_pieces(*whole, ANCHORS, capacity=64)[2])
    near_ms = median_ms(lambda: ctx.world_pieces(*near, ANCHORS | gpu.ANCHOR_OUTSIDE, capacity=64)[2])
    t = time.perf_counter()
    ctx.world_pieces(*whole, ANCHORS, capacity=64)
    whole_call_ms = (time.perf_counter() - t) * 1e3
    # the route without the call: read LOD 0 back, union-find on the host
    t = time.perf_counter()
    blob, columns = ctx.read_level(0)
    read_ms = (time.perf_counter() - t) * 1e3
    path = os.path.join(work, "world.bin")
    open(path, "wb").write(blob)
    text = subprocess.check_output([rules, "world", path, *[str(d) for d in dims], str(columns), "0", "0", "0", *[str(d) for d in dims], str(ANCHORS), "5",
                                    os.path.join(work, "list.bin"), os.path.join(work, "sub.bin")], text=True).split()
    nodes, host_ms = int(text[text.index("nodes") + 1]), float(text[text.index("ms") + 1])
    host_summary = np.frombuffer(open(os.path.join(work, "list.bin"), "rb").read()[:32], dtype=gpu.PIECES_SUMMARY_DTYPE)[0]
    assert {n: int(host_summary[n]) for n in host_summary.dtype.names} == summary, "the host route disagrees with the device"
    t = time.perf_counter()
    _, removed, remove_ms = ctx.world_pieces(*whole, ANCHORS, gpu.PIECES_REMOVE, level_count=5, capacity=0)
    remove_call_ms = (time.perf_counter() - t) * 1e3
    _, after, _ = ctx.world_pieces(*whole, ANCHORS, capacity=0)
    assert after["floatingPieces"] == 0
    print(json.dumps({"world": name, "solid_runs": nodes, "pieces": summary["floatingPieces"] + summary["anchoredPieces"], "floating": summary["floatingPieces"],
                      "floating_voxels": summary["floatingVoxels"], "report_whole_device_ms": whole_ms, "report_whole_call_ms": round(whole_call_ms, 3),
                      "report_256_box_device_ms": near_ms, "remove_device_ms": round(remove_ms, 3), "remove_call_ms": round(remove_call_ms, 3),
                      "read_level_ms": round(read_ms, 1), "host_union_find_ms": round(host_ms, 1), "host_route_ms": round(read_ms + host_ms, 1),
                      "repeats": repeats}), flush=True)
    ctx.close()


bench("mill512", scenes.load_world("mill512"))
t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
bench(f"proc{dim}", ws)
