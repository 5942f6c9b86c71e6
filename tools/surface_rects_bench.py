"""cvx_world_surface_rects on the procedural world of bench.py, and on the same world with built structure on it.
Usage: python tools/surface_rects_bench.py [dim] [repeats] [out.md] ; prints one JSON line per case and writes the table to out.md (default
profiles/surface_rects.md).

Cases: the whole procedural world and a 256 x dimY x 256 box, with and without CVX_SURFACE_IGNORE_COLOUR; then the world after brush FILL
strokes of one colour -- an 8 x 8 grid of buildings, each a 130 x 3 x 70 floor on the highest point of its footprint with two walls 40 high --
as the whole world and as a box around four of the buildings; then the same with one beam of 4 x 4 voxels along the whole of x near the top of
the world, whose faces are chains as long as the world, each walked by one thread.

Per row: the columns of the box, the strips (cvx_world_surface's quads), the rectangles and strips per rectangle, then medians of `repeats` calls
with min .. max, in device milliseconds: the count call (capacity 0), cvx_world_surface_rects_device (every rectangle left on the device), and
beside them the yardstick, cvx_world_surface's count call and cvx_world_surface_device on the same box in the same process.  The rectangles'
summary is asserted against the quads' (strips, unit faces), the rectangles' areas against the unit faces."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "surface_rects.md")
OUTSIDE = gpu.SURFACE_OUTSIDE_DEFAULT
GREY = 0xFF808080


def spread(values):
    """median (min .. max)"""
    return f"{np.median(values):.3f} ({min(values):.3f} .. {max(values):.3f})"


def timed(call):
    device, result = [], None
    for _ in range(repeats):
        result = call()
        device.append(result[-1])
    return spread(device), result


def box_stroke(lo, hi):
    return {"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": lo, "b": hi, "argb": GREY}


t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
dims = tuple(ws.dims)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
ctx = gpu.Context(0)
ctx.upload_world(ws)
side = min(256, dims[0])
corner = (dims[0] // 2 - side // 2, 0, dims[2] // 2 - side // 2)
rows = []


def measure(world, name, lo, hi):
    for flags in (0, gpu.SURFACE_IGNORE_COLOUR):
        ctx.world_surface_rects(lo, hi, OUTSIDE, flags, 0)  # (warm-up)
        count_ms, (_, summary, _) = timed(lambda: ctx.world_surface_rects(lo, hi, OUTSIDE, flags, 0))
        total = summary["rects"]
        buffer = torch.empty((max(total, 1), 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        device_ms, (device_summary, _) = timed(lambda: ctx.world_surface_rects_device(lo, hi, buffer.data_ptr(), total, OUTSIDE, flags))
        size = buffer[:total, 3:6].to(torch.int64)
        area, longest = int(size.prod(dim=1).sum()), int(size.max()) if total else 0
        del buffer, size
        quad_count_ms, (_, quads, _) = timed(lambda: ctx.world_surface(lo, hi, OUTSIDE, flags, 0))
        buffer = torch.empty((max(quads["quads"], 1), 6), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        quad_device_ms, _ = timed(lambda: ctx.world_surface_device(lo, hi, buffer.data_ptr(), quads["quads"], OUTSIDE, flags))
        del buffer
        assert device_summary == summary and (summary["strips"], summary["unitFaces"]) == (quads["quads"], quads["unitFaces"]) and area == summary["unitFaces"]
        row = {"world": world, "box": name, "flags": flags, "columns": (hi[0] - lo[0]) * (hi[2] - lo[2]), "strips": summary["strips"], "rects": total,
               "strips_per_rect": round(summary["strips"] / max(total, 1), 2), "longest_side": longest, "rects_count_ms": count_ms, "rects_device_ms": device_ms,
               "surface_count_ms": quad_count_ms, "surface_device_ms": quad_device_ms}
        rows.append(row)
        print(json.dumps(row), flush=True)


measure("procedural", "whole world", (0, 0, 0), dims)
measure("procedural", f"{side} x {dims[1]} x {side} box", corner, (corner[0] + side, dims[1], corner[2] + side))

# built structure: buildings on the terrain
pitch, first = dims[0] // 8, dims[0] // 16 - 65
strokes = []
for i in range(8):
    for j in range(8):
        x, z = first + i * pitch, first + j * pitch
        heights, _, _ = ctx.read_heights((x, 0, z), (x + 130, dims[1], z + 70), want_argb=False)
        y = min(int(heights.max()), dims[1] - 64)
        strokes += [box_stroke((x, y, z), (x + 130, y + 3, z + 70)), box_stroke((x, y + 3, z), (x + 130, y + 43, z + 2)), box_stroke((x, y + 3, z), (x + 2, y + 43, z + 70))]
ctx.brush(strokes)
measure("with 64 buildings", "whole world", (0, 0, 0), dims)
measure("with 64 buildings", "box around four buildings", (first - 8, 0, first - 8), (first + pitch + 138, dims[1], first + pitch + 78))
ctx.brush([box_stroke((0, dims[1] - 12, dims[2] // 2), (dims[0], dims[1] - 8, dims[2] // 2 + 4))])
measure("... and a beam along all of x", "whole world", (0, 0, 0), dims)
ctx.close()

names = list(rows[0])
with open(out_path, "w") as fh:
    fh.write(f"# cvx_world_surface_rects, cvx_world_surface_rects_device: tools/surface_rects_bench.py {dim} {repeats}\n\n")
    fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}), solidOutside CVX_SURFACE_OUTSIDE_DEFAULT; flags 1 = CVX_SURFACE_IGNORE_COLOUR; medians of {repeats} "
             "calls with min .. max, device milliseconds.  rects_count = cvx_world_surface_rects with capacity 0; rects_device = cvx_world_surface_rects_device, every "
             "rectangle left on the device; surface_count / surface_device = cvx_world_surface with capacity 0 / cvx_world_surface_device on the same box in the same "
             "process: the yardstick.  longest_side = the largest extent of a rectangle, in voxels.\n\n")
    fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
    for row in rows:
        fh.write("| " + " | ".join(str(row[n]) for n in names) + " |\n")
