"""cvx_world_settle on mill512 and on the procedural world of bench.py, after one sphere carve; and on the stack of twelve slabs of the tests.
Usage: python tools/settle_bench.py [dim] [repeats] ; prints one JSON line per scene.  Needs the experiment build (make gpu-exp): the split of the
device time and the sweep count come from cvx_debug_settle (include/cpuvox_gpu_diag.h).

Per world, over a 256^3 box around the carve with anchors = 0 (every piece of the box floats; what the box's bottom cuts holds still), medians of
`repeats` with the spread (min .. max): a REPORT of the same box; the settle, split into analysis, gap + relax (with its sweeps and launches) and
edit; the same with ONE sweep per launch (the comparison variant of the relax loop); the REMOVE of the same call.  The world is put back between
repeats from a cvx_world_read_region copy of the box's footprint.  Beside them the route a host had before this call, timed in the same run:
cvx_world_read_level of LOD 0, the rules on the host (tests/settle_rules.cpp: union-find, Bellman-Ford, column emitter), cvx_world_edit of the
rectangle -- and its world compared byte for byte with the device's."""
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
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
gpu.use_library(os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu_exp.so"))
work = tempfile.mkdtemp(prefix="settle_bench")
rules = ruleslib.build("settle_rules", work, "-O2")


def stat(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(min(values)), 3), "max": round(float(max(values)), 3)}


def settle_runs(ctx, box, anchors, footprint, saved, one_sweep):
    """`repeats` settles of the same world (put back in between) -> the medians of the total and its three parts, and the last call's counts."""
    ctx.debug_settle(1 if one_sweep else 0)
    rows = []
    for _ in range(repeats + 1):  # (the first one warms up)
        _, _, summary, ms = ctx.world_settle(*box, anchors, capacity=0)
        d = ctx.debug_settle()
        rows.append((ms, d["analysis_ms"], d["relax_ms"], d["edit_ms"]))
        if summary["fallenPieces"]:
            ctx.edit(*footprint, saved, footprint[2] * footprint[3])
    ctx.debug_settle(0)
    rows = np.array(rows[1:])
    return ({"device_ms": stat(rows[:, 0]), "analysis_ms": stat(rows[:, 1]), "gap_relax_ms": stat(rows[:, 2]), "edit_ms": stat(rows[:, 3]), "sweeps": d["sweeps"],
             "launches": d["launches"], "single_workgroup": d["single_workgroup"]}, summary)


def bench(name, ws, box=None, anchors=0, carve=True):
    dims = tuple(ws.dims)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    if carve:  # a sphere around a surface voxel near the middle of the world
        o = np.array([[dims[0] * 0.5 + 0.5, dims[1] - 0.5, dims[2] * 0.5 + 0.5]])
        vox, face, _, _ = ctx.pick(o, np.array([[0.0, -1.0, 0.0]]), float(dims[1]))
        centre = [int(v) for v in vox[0]] if face[0] >= 0 else [dims[0] // 2, dims[1] // 4, dims[2] // 2]
        ctx.brush([{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_SPHERE, "a": centre, "radius": min(48, dims[0] // 8)}], 5)
        box = ([max(0, c - 128) for c in centre], [min(c + 128, d) for c, d in zip(centre, dims)])
    # the box's footprint rounded outward to 32 columns: what a settle or a REMOVE inside it can touch
    x0, z0 = box[0][0] & ~31, box[0][2] & ~31
    x1, z1 = min((box[1][0] + 31) & ~31, dims[0]), min((box[1][2] + 31) & ~31, dims[2])
    footprint = (x0, z0, x1 - x0, z1 - z0)
    saved, _ = ctx.read_region(0, *footprint)
    before, columns = ctx.read_level(0)
    report = [ctx.world_pieces(*box, anchors, capacity=0)[2] for _ in range(repeats + 1)][1:]
    batched, summary = settle_runs(ctx, box, anchors, footprint, saved, one_sweep=False)
    single, _ = settle_runs(ctx, box, anchors, footprint, saved, one_sweep=True)
    removes = []
    for _ in range(repeats + 1):
        removes.append(ctx.world_pieces(*box, anchors, gpu.PIECES_REMOVE, capacity=0)[2])
        ctx.edit(*footprint, saved, footprint[2] * footprint[3])
    assert ctx.read_level(0)[0] == before, "putting the footprint back did not restore the world"
    # the device's result
    t = time.perf_counter()
    ctx.world_settle(*box, anchors, capacity=0)
    call_ms = (time.perf_counter() - t) * 1e3
    device_world = ctx.read_level(0)[0]
    ctx.edit(*footprint, saved, footprint[2] * footprint[3])
    # the route without the call: read LOD 0 back, the rules on the host, cvx_world_edit
    t = time.perf_counter()
    blob, columns = ctx.read_level(0)
    read_ms = (time.perf_counter() - t) * 1e3
    path = os.path.join(work, "world.bin")
    open(path, "wb").write(blob)
    text = subprocess.check_output([rules, "world", path, *[str(d) for d in dims], str(columns), *[str(v) for v in box[0]], *[str(v) for v in box[1]], str(anchors), "0", "5",
                                    os.path.join(work, "list.bin"), os.path.join(work, "sub.bin")], text=True).split()
    rect = [int(v) for v in text[text.index("rect") + 1:text.index("rect") + 5]]
    host_ms, host_sweeps = float(text[text.index("ms") + 1]), int(text[text.index("sweeps") + 1])
    edit_ms = 0.0
    if summary["fallenPieces"]:
        t = time.perf_counter()
        ctx.edit(*rect, open(os.path.join(work, "sub.bin"), "rb").read(), rect[2] * rect[3])
        edit_ms = (time.perf_counter() - t) * 1e3
    same = ctx.read_level(0)[0] == device_world
    print(json.dumps({"scene": name, "box": box, "anchors": anchors, "solid_runs": int(text[text.index("nodes") + 1]), **summary,
                      "report_device_ms": stat(report), "settle": batched, "settle_one_sweep_per_launch": single, "remove_device_ms": stat(removes[1:]),
                      "settle_call_ms": round(call_ms, 3), "host_read_level_ms": round(read_ms, 1), "host_rules_ms": round(host_ms, 1), "host_rules_sweeps": host_sweeps,
                      "host_edit_call_ms": round(edit_ms, 1), "host_route_ms": round(read_ms + host_ms + edit_ms, 1), "host_route_world_identical": same,
                      "repeats": repeats}), flush=True)
    assert same, "the host route and the device disagree"
    ctx.close()


def stack(dims):
    """The tests' stack: slab k lies k voxels above slab k - 1 over a floor, twelve of them."""
    solid = np.zeros(dims, dtype=bool)
    solid[:, 0, :] = True
    y = 0
    for k in range(1, 13):
        y += k + 1
        solid[60:64, y, 60:64] = True
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), np.full(len(x), 0xFF808080, dtype=np.uint32), threads=4)


bench("stack of 12, one workgroup", stack((128, 128, 128)), box=([56, 0, 56], [72, 128, 72]), anchors=gpu.ANCHOR_GROUND, carve=False)
bench("stack of 12, whole world", stack((128, 128, 128)), box=([0, 0, 0], [128, 128, 128]), anchors=gpu.ANCHOR_GROUND, carve=False)
bench("mill512", scenes.load_world("mill512"))
t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
print(json.dumps({"scene": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
bench(f"proc{dim}", ws)
