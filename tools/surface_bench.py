"""cvx_world_surface on the procedural world of bench.py: the whole world and a 256 x dimY x 256 box, with and without CVX_SURFACE_IGNORE_COLOUR.
Usage: python tools/surface_bench.py [dim] [repeats] [out.md] ; prints one JSON line per (box, flags) and writes the table to out.md (default
profiles/surface.md).

Per row: the columns of the box, the quads and the exposed voxel faces, then medians of `repeats` calls with min .. max, in milliseconds: the
device time and the wall-clock time of the count call (capacity 0), of the full call with the quads copied to the host, and of
cvx_world_surface_device, which leaves them on the device; and beside them the route a host has without this call, timed in the same run:
cvx_world_read_level of LOD 0 plus the walk of cvx_surface.h over the blob on one host core (tests/surface_rules.cpp, its own milliseconds
without loading the blob).  The summaries and the quads of the two routes are asserted equal, byte for byte."""
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
import torch  # noqa: E402
import ruleslib  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "surface.md")
work = tempfile.mkdtemp(prefix="surface_bench")
rules = ruleslib.build("surface_rules", work, "-O2")


def spread(values):
    """median (min .. max)"""
    return f"{np.median(values):.3f} ({min(values):.3f} .. {max(values):.3f})"


def timed(call):
    device, wall, result = [], [], None
    for _ in range(repeats):
        t = time.perf_counter()
        result = call()
        wall.append((time.perf_counter() - t) * 1e3)
        device.append(result[-1])
    return spread(device), spread(wall), result


t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
dims = tuple(ws.dims)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
ctx = gpu.Context(0)
ctx.upload_world(ws)
t = time.perf_counter()
blob, columns = ctx.read_level(0)
read_ms = (time.perf_counter() - t) * 1e3
path = os.path.join(work, "world.bin")
open(path, "wb").write(blob)
del blob
side = min(256, dims[0])
corner = (dims[0] // 2 - side // 2, 0, dims[2] // 2 - side // 2)
boxes = [("whole world", (0, 0, 0), dims), (f"{side} x {dims[1]} x {side} box", corner, (corner[0] + side, dims[1], corner[2] + side))]
OUTSIDE = gpu.SURFACE_OUTSIDE_DEFAULT
rows = []
for name, lo, hi in boxes:
    for flags in (0, gpu.SURFACE_IGNORE_COLOUR):
        ctx.world_surface(lo, hi, OUTSIDE, flags, 0)  # (warm-up)
        count_device, count_wall, (_, summary, _) = timed(lambda: ctx.world_surface(lo, hi, OUTSIDE, flags, 0))
        total = summary["quads"]
        full_device, full_wall, (quads, full_summary, _) = timed(lambda: ctx.world_surface(lo, hi, OUTSIDE, flags, total))
        buffer = torch.empty((max(total, 1), 6), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        stay_device, stay_wall, (stay_summary, _) = timed(lambda: ctx.world_surface_device(lo, hi, buffer.data_ptr(), total, OUTSIDE, flags))
        assert full_summary == summary == stay_summary and len(quads) == total
        assert buffer[:total].cpu().numpy().tobytes() == quads.tobytes(), "the device variant's quads differ from the host variant's"
        del buffer
        # the route without the call: LOD 0 read back (once, above), the same walk on one host core
        listing = os.path.join(work, "quads.bin")
        text = subprocess.check_output([rules, "world", path, *[str(d) for d in dims], str(columns), *[str(v) for v in lo], *[str(v) for v in hi], str(OUTSIDE), str(flags),
                                        listing], text=True).split()
        host_ms = float(text[text.index("ms") + 1])
        raw = np.fromfile(listing, dtype=np.uint8)
        host_summary = raw[:64].view(gpu.SURFACE_SUMMARY_DTYPE)[0]
        assert int(host_summary["quads"]) == total and int(host_summary["unitFaces"]) == summary["unitFaces"], "the host route disagrees with the device"
        assert raw[64:].tobytes() == quads.tobytes(), "the host route's quads differ from the device's"
        row = {"box": name, "flags": flags, "columns": (hi[0] - lo[0]) * (hi[2] - lo[2]), "quads": total, "unit_faces": summary["unitFaces"],
               "count_device_ms": count_device, "count_call_ms": count_wall, "full_device_ms": full_device, "full_call_ms": full_wall,
               "device_variant_device_ms": stay_device, "device_variant_call_ms": stay_wall,
               "read_level_ms": round(read_ms, 1), "host_walk_ms": round(host_ms, 1), "host_route_ms": round(read_ms + host_ms, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del quads, raw
ctx.close()

names = list(rows[0])
with open(out_path, "w") as fh:
    fh.write(f"# cvx_world_surface, cvx_world_surface_device: tools/surface_bench.py {dim} {repeats}\n\n")
    fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}), solidOutside CVX_SURFACE_OUTSIDE_DEFAULT; flags 1 = CVX_SURFACE_IGNORE_COLOUR; medians of {repeats} "
             "calls with min .. max, milliseconds.  count = capacity 0; full = every quad copied to the host; device_variant = every quad left on the device.  "
             "The host route is cvx_world_read_level of LOD 0 plus the walk of cvx_surface.h on one host core; its summary and quads equal the device's byte for byte.\n\n")
    fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
    for row in rows:
        fh.write("| " + " | ".join(str(row[n]) for n in names) + " |\n")
