"""cvxd_models_brush_device on bodies lifted from the procedural world of bench.py, beside the only route there was before it: FILL the bodies
into an empty scratch region of the world, brush the world there, and read every body back through the inverse of its map
(cvx_world_place_models_device, cvx_world_brush, one cvx_world_read_model_device a body).
Usage: python tools/model_brush_bench.py [dim] [repeats] [out.md] ; prints one JSON line per case and writes the table to out.md (default
profiles/model_brush.md; the compiler's figures at its head are COMPILER below, taken from the build).

Bodies: tools/pair_contacts_bench.py's -- 32 x 32 loose chunks of 7 x 4 x 7 voxels lifted with cvx_world_lift_pieces_device into torch pools, body
k the model k under a yaw and a tilt of its own -- in tools/pair_sweep_bench.py's loose pile (12 x 8 x 12 voxels a cell), set into the 64 voxels
under the world's top, which a CARVE has emptied: the scratch region of the route is the pile's own place.
Cases: one CARVE sphere through the pile of 256 bodies; 64 strokes (spheres and capsules, CARVE and PAINT) through the pile; one body, one sphere.
The route is given its best form: ONE place call for all bodies, ONE brush, then a read-back a body; the carve that empties the region again is
not timed.  Both routes start every round from the same arrays (the pools are restored from a copy before each, untimed).
Before timing, the two routes' arrays are compared voxel by voxel and the differences counted: the read-back samples the world at the image of
each model voxel's centre, the call changes the model voxels that the body's world voxels map to, and the two maps are each other's rounded
inverses, not each other's inverses.
Columns (milliseconds are medians over `repeats` rounds after a warm-up round, with min .. max):
  call device / wall ms   cvxd_models_brush_device's own device time (outDeviceMs) and the host clock around it
  route wall ms           the host clock around place + brush + the read-backs and a final synchronisation
  route device ms         the device time place and brush report (the read-backs report none)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402
from contacts_bench import CORNER, box, cell, chunk_strokes, rotation, stat  # noqa: E402

COMPILER = """# cvxd_models_brush: the compiler's figures and the measured cost (tools/model_brush_bench.py)

## The kernels as compiled for gfx950

`hipcc -Rpass-analysis=kernel-resource-usage` on cvx_model_brush.hip with the Makefile's flags:

| kernel | VGPRs | SGPRs | SGPR spills (to VGPR lanes) | scratch bytes / lane | LDS bytes | occupancy, waves / SIMD |
|---|---|---|---|---|---|---|
| `brush_cull_kernel` | 38 | 44 | 0 | 0 | 0 | 8 |
| `brush_mark_kernel` | 36 | 106 | 49 | 0 | 0 | 7 |
| `brush_apply_kernel` | 92 | 58 | 0 | 0 | 0 | 5 |

No scratch and no LDS.  The mark kernel keeps the instance's column job, the list word and the stroke in scalar registers; a lane holds its
voxel's y, its element and its key.  The apply kernel's registers are a lane's nine 64-bit sums, three counts and the box; it is bound by the
loads of the key array and the models' arrays (9 bytes a voxel of a model with colours and a mask).
"""
CARVE, PAINT, FILL = gpu.BRUSH_CARVE, gpu.BRUSH_PAINT, gpu.BRUSH_FILL


def pile(count, sizes, rng, lift):
    """tools/pair_sweep_bench.py's loose pile, `lift` voxels up: (instances, body k's map back into the world for the read-back)."""
    side = int(np.ceil(count ** (1 / 3)))
    instances, back = [], []
    for k in range(count):
        size = sizes[k % len(sizes)]
        gx, gz, gy = k % side, (k // side) % side, k // (side * side)
        centre = np.array([16 + 12 * gx, lift + 8 + 8 * gy, 16 + 12 * gz], dtype=np.float64) + rng.uniform(-1, 1, 3)
        linear = rotation(1, float(rng.uniform(0, 360))) @ rotation(0, float(rng.uniform(-20, 20)))
        forward = np.concatenate([linear, (centre - linear @ (np.asarray(size, dtype=np.float64) / 2))[:, None]], axis=1)
        instances.append(gpu.model_instance(forward, size, k % len(sizes), FILL))
        inverse = np.linalg.inv(np.concatenate([forward, [[0.0, 0.0, 0.0, 1.0]]], axis=0))[:3]
        back.append(gpu.model_instance(inverse, size).toModel)
    return instances, back


def strokes_of(case, instances, rng):
    lo = np.min([list(i.boxMin) for i in instances], axis=0)
    hi = np.max([list(i.boxMax) for i in instances], axis=0)
    mid = [int(v) for v in (lo + hi) // 2]
    if case != "64 strokes":
        return [{"op": CARVE, "shape": gpu.SHAPE_SPHERE, "a": mid, "b": [int(min(hi - lo) // 3) if case == "one sphere" else 3, 0, 0], "argb": 0}]
    strokes = []
    for j in range(64):
        a = [int(rng.integers(lo[i], hi[i])) for i in range(3)]
        op = CARVE if j % 3 == 0 else PAINT
        argb = 0 if op == CARVE else 0xFF000100 + j
        if j % 2:
            strokes.append({"op": op, "shape": gpu.SHAPE_CAPSULE, "a": a, "b": [a[i] + int(rng.integers(-20, 21)) for i in range(3)], "radius": 3, "argb": argb})
        else:
            strokes.append({"op": op, "shape": gpu.SHAPE_SPHERE, "a": a, "b": [int(rng.integers(3, 9)), 0, 0], "argb": argb})
    return strokes


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "model_brush.md")
    ws = host.WorldSet.procedural(dim, dim, dim)
    ctx = gpu.Context(0)
    rows = []
    try:
        ctx.upload_world(ws)
        y0 = dim - 64
        ctx.brush(chunk_strokes(y0), 5)
        lift_box = ((0, y0 - 1, 0), (CORNER, y0 + 5, CORNER))
        _, totals, _ = ctx.world_lift_pieces_device(*lift_box, gpu.ANCHOR_GROUND, None, None, capacity=0)
        argb = torch.zeros(totals["neededVoxels"], dtype=torch.int32, device="cuda")
        mask = torch.zeros(totals["neededVoxels"], dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pieces, totals, _ = ctx.world_lift_pieces_device(*lift_box, gpu.ANCHOR_GROUND, argb, mask, gpu.LIFT_REMOVE, capacity=1024)
        assert totals["storedPieces"] == 1024 == len(pieces)
        region = box(CARVE, (0, y0 - 2, 0), (CORNER + 1, dim, CORNER + 1))
        ctx.brush([region], 0)  # the scratch region: the pile's place, empty
        model_count = gpu.MODELS_MAX_MODELS
        descriptors = [gpu.lifted_model(pieces, k, argb.data_ptr(), mask.data_ptr()) for k in range(model_count)]
        argb_kept, mask_kept = argb.clone(), mask.clone()
        rng = np.random.default_rng(2048)
        for case, count in (("one sphere", 256), ("64 strokes", 256), ("one body", 1)):
            instances, back = pile(count, [d[0] for d in descriptors], rng, y0)
            assert max(i.boxMax[1] for i in instances) < dim and min(i.boxMin[1] for i in instances) > y0 and max(max(i.boxMax[0], i.boxMax[2]) for i in instances) < CORNER
            strokes = gpu.strokes_array(strokes_of(case, instances, rng))
            models = descriptors[:count]
            tensors = []  # the call's form of the same pools: a view a model
            for size, a_ptr, m_ptr in models:
                n = size[0] * size[1] * size[2]
                at = (a_ptr - argb.data_ptr()) // 4
                tensors.append((argb[at:at + n].view(size[0], size[2], size[1]), mask[at:at + n].view(size[0], size[2], size[1])))
            route_argb, route_mask = torch.zeros_like(argb), torch.zeros_like(mask)
            inst = gpu._instance_array(instances)
            call_device, call_wall, route_wall, route_device = [], [], [], []
            differ = None
            for r in range(repeats + 1):
                argb.copy_(argb_kept)
                mask.copy_(mask_kept)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                placed_ms = ctx.place_models_device(models, inst, 0)
                brushed_ms = ctx.brush(strokes, 0)
                for (size, a_ptr, m_ptr), to_world in zip(models, back):
                    ctx.read_model_device(size, to_world, route_argb.data_ptr() + (a_ptr - argb.data_ptr()), route_mask.data_ptr() + (m_ptr - mask.data_ptr()))
                torch.cuda.synchronize()
                took = (time.perf_counter() - t0) * 1000.0
                ctx.brush([region], 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                results, hit, summary, ms = ctx.models_brush_device(tensors, inst, strokes)
                wall = (time.perf_counter() - t0) * 1000.0
                if r == 0:  # where the two routes' answers differ
                    used = sum(s[0] * s[1] * s[2] for s, _, _ in models)
                    first = (models[0][1] - argb.data_ptr()) // 4
                    mine, theirs = mask[first:first + used] != 0, route_mask[first:first + used] != 0
                    colours = (argb[first:first + used] != route_argb[first:first + used]) & mine & theirs
                    differ = {"voxels": used, "set_by_the_call_only": int((mine & ~theirs).sum()), "set_by_the_route_only": int((theirs & ~mine).sum()),
                              "both_set_other_colour": int(colours.sum()), "left_by_the_call": int(mine.sum()), "left_by_the_route": int(theirs.sum())}
                else:
                    call_device.append(ms)
                    call_wall.append(wall)
                    route_wall.append(took)
                    route_device.append(placed_ms + brushed_ms)
            row = {"case": case, "bodies": count, "strokes": len(strokes), "jobs": summary["jobs"], "carved": summary["carved"], "painted": summary["painted"],
                   "bodies_hit": int(((hit["carved"] + hit["painted"]) > 0).sum()), "call_device_ms": stat(call_device), "call_wall_ms": stat(call_wall),
                   "route_wall_ms": stat(route_wall), "route_device_ms": stat(route_device), "differ": differ}
            row["ratio"] = row["route_wall_ms"]["median"] / row["call_wall_ms"]["median"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        ctx.close()
        ws.close()
    lines = [COMPILER, "## Measured", "",
             f"Produced by `python tools/model_brush_bench.py {dim} {repeats}` on one {torch.cuda.get_device_name(0)}: bodies lifted from the procedural world {dim}^3 in a "
             f"loose pile, medians of {repeats} interleaved rounds after a warm-up round (min .. max).  The route is one place call for all bodies, one brush and a "
             "read-back a body; no time was fixed beforehand for either side.", "",
             "| case | bodies | strokes | jobs | bodies hit | carved | painted | call device ms | call wall ms | route wall ms | route device ms (place + brush) | route / call, wall |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        lines.append(f"| {row['case']} | {row['bodies']} | {row['strokes']} | {row['jobs']} | {row['bodies_hit']} | {row['carved']} | {row['painted']} | {cell(row['call_device_ms'])} | "
                     f"{cell(row['call_wall_ms'])} | {cell(row['route_wall_ms'])} | {cell(row['route_device_ms'])} | {row['ratio']:.1f} |")
    lines += ["", "## Where the route's answer differs", "",
              "The two routes were run on the same arrays and compared voxel by voxel before timing.  The call changes the model voxels that the body's WORLD voxels map "
              "to (toModel of every voxel of the box); the route rasterises the body into the world with the same map, brushes the world, and then samples the world at the "
              "image of every MODEL voxel's centre under the rounded inverse map.  Under a rotation the two are not the same set: a model voxel whose centre falls into a "
              "world voxel that another model voxel filled, or that no body voxel maps from, reads back what that world voxel holds.", "",
              "| case | model voxels | left set by the call | left set by the route | set by the call only | set by the route only | both set, other colour |", "|---|---|---|---|---|---|---|"]
    for row in rows:
        d = row["differ"]
        lines.append(f"| {row['case']} | {d['voxels']} | {d['left_by_the_call']} | {d['left_by_the_route']} | {d['set_by_the_call_only']} | {d['set_by_the_route_only']} | "
                     f"{d['both_set_other_colour']} |")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
