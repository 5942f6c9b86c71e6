"""cvx_world_distance_device on the procedural world of bench.py: a 256^3 box across the terrain's surface in the middle of the world, for
R = 4, 16, 64, 255 and the three modes, beside cvx_world_read_voxels_device of the same box as the floor.
Usage: python tools/distance_bench.py [dim] [repeats] [out.md] ; prints one JSON line per measurement and writes the table to out.md (default
profiles/distance.md).

  distance_ms   the call's own device time (outDeviceMs: events around its kernels on the context's stream), into a torch int32 tensor; the median
                of `repeats` calls after one warm-up call, with min .. max
  Gvoxels/s     the box's voxels over that time
  floor_ms      cvx_world_read_voxels_device of the same box into a torch int32 tensor (argb alone), timed with events on the stream it is
                enqueued on: it reads the same arena with a binary search per element and writes the same number of 4-byte elements, with no
                halo, no intermediate arrays and no scan
  x floor       distance_ms / floor_ms
  scratch_MB    the call's device memory while it runs (the formula of include/cpuvox_gpu.h)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

RADII = (4, 16, 64, 255)
MODES = (("TO_SOLID", gpu.DISTANCE_TO_SOLID), ("TO_AIR", gpu.DISTANCE_TO_AIR), ("SIGNED", gpu.DISTANCE_SIGNED))


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "distance.md")
    t0 = time.perf_counter()
    ws = host.WorldSet.procedural(dim, dim, dim)
    dims = tuple(ws.dims)
    print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    # the terrain's surface in the middle of the world: the box straddles it
    _, column = ctx.read_voxels((dims[0] // 2, 0, dims[2] // 2), (dims[0] // 2 + 1, dims[1], dims[2] // 2 + 1), want_argb=False)
    surface = int(np.nonzero(column[0, 0])[0].max()) + 1 if column.any() else dims[1] // 2
    side = min(256, dims[0])
    lo = (dims[0] // 2 - side // 2, max(0, min(dims[1] - side, surface - side // 2)), dims[2] // 2 - side // 2)
    hi = (lo[0] + side, lo[1] + side, lo[2] + side)
    shape = (side, side, side)
    voxels = side ** 3
    out = torch.empty(shape, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()  # (a stream of its own: torch's default stream has the handle 0, which the call reads as "the context's")
    torch.cuda.synchronize()

    def floor():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            a.record(stream)
            ctx.read_voxels_device(lo, hi, out.data_ptr(), 0, stream.cuda_stream)
            b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    floor()  # (warm-up)
    floor_ms = float(np.median([floor() for _ in range(max(repeats, 5))]))
    solid_fraction = float((out != 0).float().mean().item())
    print(json.dumps({"box": [list(lo), list(hi)], "surface_y": surface, "voxels": voxels, "solid_fraction": round(solid_fraction, 3), "floor_ms": round(floor_ms, 4)}), flush=True)
    rows = []
    for R in RADII:
        scratch = 2 * side * (side + 2 * R) * (2 * side + 2 * R)
        for name, mode in MODES:
            ctx.distance_device(lo, hi, R, out.data_ptr(), mode)  # (warm-up)
            ms = [ctx.distance_device(lo, hi, R, out.data_ptr(), mode) for _ in range(repeats)]
            median = float(np.median(ms))
            far = float((out.abs() == gpu.DISTANCE_FAR).float().mean().item())
            row = {"R": R, "mode": name, "distance_ms": round(median, 3), "min .. max": f"{min(ms):.3f} .. {max(ms):.3f}", "Gvoxels/s": round(voxels / median / 1e6, 2),
                   "floor_ms": round(floor_ms, 4), "x floor": round(median / floor_ms, 1), "scratch_MB": round(scratch / 1e6, 1), "far_fraction": round(far, 3)}
            rows.append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    with open(out_path, "w") as fh:
        fh.write(f"# cvx_world_distance: tools/distance_bench.py {dim} {repeats}\n\n")
        fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}) on one MI355X; the box {list(lo)} .. {list(hi)} ({side}^3 = {voxels} voxels, {solid_fraction:.1%} solid) "
                 f"straddles the terrain's surface (y = {surface}) in the middle of the world.  `distance_ms`: cvx_world_distance_device into a torch int32 tensor, the call's "
                 f"own device time (events around its kernels), median of {repeats} calls after one warm-up call, with min .. max.  `floor_ms`: "
                 f"cvx_world_read_voxels_device of the same box into the same tensor (argb alone: the same arena, a binary search per element, the same number of "
                 f"4-byte elements written), events on its stream, median of {max(repeats, 5)} calls after a warm-up.  `x floor` = distance_ms / floor_ms.  `scratch_MB`: the "
                 f"two 16-bit intermediate arrays.  `far_fraction`: the part of the box that came out CVX_DISTANCE_FAR.  No threshold is set on any of these.\n\n")
        names = list(rows[0])
        fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
        for row in rows:
            fh.write("| " + " | ".join(str(row[n]) for n in names) + " |\n")


if __name__ == "__main__":
    main()
