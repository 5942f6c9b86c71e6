"""cvx_world_spread_device on the procedural world of bench.py, beside what a user has to do without the call: cvx_world_read_voxels_device of the
same box and a level-synchronous torch loop on the device (shifted logical_ors masked by passability, one pass over the box per step), which
produces the same field -- the tool compares the bytes.
Usage: python tools/spread_bench.py [dim] [repeats] [out.md] ; prints one JSON line per case and writes the table to out.md (default
profiles/spread.md).

Cases, all over a 512 x 64 x 512 box across the terrain's surface in the middle of the world:
  air 64 / air 1024   AIR, every direction, 64 seeds on a grid at the box's top, maxSteps 64 and 1024
  pond                AIR, 0x37 (no step up), one spring just above the ground in the middle, the box's top lowered to the spring, maxSteps 64: a
                      small reached region in the same footprint -- what the active flags are for
  flood               the same at maxSteps 4096: the procedural world is a shell, and the water runs on under it
  solid               SOLID, every direction, up to 4096 seeds on a 64 x 64 grid, each on the lowest solid voxel of its column inside the box (the ground
                      up), maxSteps 1024; the procedural world is a thin shell, so little of the box is solid
Columns:
  spread_ms      the call's own device time (outDeviceMs: events around everything it enqueues, the host's reads of the changed flag between the
                 launches included), median of `repeats` calls after a warm-up call, with min .. max
  launches, tileVisits, reached   the call's summary; ms/Mreached = spread_ms per million reached voxels
  flag_ms        launches x the measured round trip of one 4-byte device-to-host copy and stream synchronise: an estimate of the part of spread_ms
                 that is the host's per-launch flag read
  torch_ms       the read of the box's solid mask and the torch loop, events around both, median of min(repeats, 3) runs; steps = its passes
  working_MB     the call's per-voxel working set (2 bytes a voxel and a passable bit); pass_ms = torch_ms / steps, one torch pass over the box"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

SHIFTS = ((0, -1), (0, 1), (2, -1), (2, 1), (1, -1), (1, 1))  # face f: (tensor axis of (X, Z, Y), direction)


def torch_field(ctx, lo, hi, shape, seeds, medium, faces, max_steps, stream):
    """What a user does today: the solid mask of the box, then one dilation per step.  -> (field, steps)."""
    solid = torch.empty(shape, dtype=torch.uint8, device="cuda")
    ctx.read_voxels_device(lo, hi, 0, solid.data_ptr(), stream.cuda_stream)
    passable = (solid != 0) if medium == gpu.SPREAD_SOLID else (solid == 0)
    dist = torch.full(shape, gpu.SPREAD_UNREACHED, dtype=torch.int32, device="cuda")
    front = torch.zeros(shape, dtype=torch.bool, device="cuda")
    s = torch.as_tensor(np.array([[x - lo[0], z - lo[2], y - lo[1]] for x, y, z in seeds]), device="cuda")
    front[s[:, 0], s[:, 1], s[:, 2]] = True
    front &= passable
    dist[front] = 0
    steps = 0
    for step in range(1, max_steps + 1):
        grown = torch.zeros_like(front)
        for f, (axis, d) in enumerate(SHIFTS):
            if not (faces >> f) & 1:
                continue
            src = [slice(None)] * 3
            dst = [slice(None)] * 3
            src[axis], dst[axis] = (slice(1, None), slice(0, -1)) if d < 0 else (slice(0, -1), slice(1, None))
            grown[tuple(dst)] |= front[tuple(src)]
        front = grown & passable & (dist < 0)
        steps = step
        if not bool(front.any()):  # (one read a step, as the call reads its flag once a launch)
            break
        dist[front] = step
    return torch.where(passable, dist, torch.full_like(dist, gpu.SPREAD_BLOCKED)), steps


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "spread.md")
    t0 = time.perf_counter()
    ws = host.WorldSet.procedural(dim, dim, dim)
    dims = tuple(ws.dims)
    print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    cx, cz = dims[0] // 2, dims[2] // 2
    _, column = ctx.read_voxels((cx, 0, cz), (cx + 1, dims[1], cz + 1), want_argb=False)
    surface = int(np.nonzero(column[0, 0])[0].max()) + 1 if column.any() else dims[1] // 2
    side, height = min(512, dims[0]), 64
    y0 = max(0, min(dims[1] - height, surface - height // 4))
    lo, hi = (cx - side // 2, y0, cz - side // 2), (cx + side // 2, y0 + height, cz + side // 2)
    grid = [(lo[0] + side // 16 + i * (side // 8), lo[2] + side // 16 + k * (side // 8)) for i in range(8) for k in range(8)]
    _, mask = ctx.read_voxels(lo, hi, want_argb=False)
    fine = [(lo[0] + side // 128 + i * (side // 64), lo[2] + side // 128 + k * (side // 64)) for i in range(64) for k in range(64)]
    ground = [(x, lo[1] + int(np.nonzero(mask[x - lo[0], z - lo[2]])[0].min()), z) for x, z in fine if mask[x - lo[0], z - lo[2]].any()]
    del mask
    cases = [
        ("air 64", lo, hi, [(x, hi[1] - 1, z) for x, z in grid], gpu.SPREAD_AIR, 0x3F, 64),
        ("air 1024", lo, hi, [(x, hi[1] - 1, z) for x, z in grid], gpu.SPREAD_AIR, 0x3F, 1024),
        ("pond", lo, (hi[0], surface + 1, hi[2]), [(cx, surface, cz)], gpu.SPREAD_AIR, 0x37, 64),
        ("flood", lo, (hi[0], surface + 1, hi[2]), [(cx, surface, cz)], gpu.SPREAD_AIR, 0x37, 4096),
        ("solid", lo, hi, ground, gpu.SPREAD_SOLID, 0x3F, 1024),
    ]
    stream = torch.cuda.Stream()  # (a stream of its own: torch's default stream has the handle 0, which the call reads as "the context's")
    probe = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        probe.cpu()
    round_trip_ms = (time.perf_counter() - t0) * 1000 / 200
    print(json.dumps({"box": [list(lo), list(hi)], "surface_y": surface, "flag_round_trip_ms": round(round_trip_ms, 4)}), flush=True)
    rows = []
    for name, b0, b1, seeds, medium, faces, max_steps in cases:
        shape = (b1[0] - b0[0], b1[2] - b0[2], b1[1] - b0[1])
        voxels = shape[0] * shape[1] * shape[2]
        out = torch.empty(shape, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.world_spread_device(b0, b1, seeds, out, medium=medium, step_faces=faces, max_steps=max_steps)  # (warm-up)
        runs = [ctx.world_spread_device(b0, b1, seeds, out, medium=medium, step_faces=faces, max_steps=max_steps) for _ in range(repeats)]
        ms = [r[1] for r in runs]
        summary, median = runs[-1][0], float(np.median(ms))
        torch_ms, steps, same = [], 0, True
        for _ in range(min(repeats, 3)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                field, steps = torch_field(ctx, b0, b1, shape, seeds, medium, faces, max_steps, stream)
                b.record(stream)
            stream.synchronize()
            torch_ms.append(a.elapsed_time(b))
            same = same and bool(torch.equal(field, out))
        t_med = float(np.median(torch_ms))
        reached = summary["reached"]
        row = {"case": name, "voxels": voxels, "maxSteps": max_steps, "spread_ms": round(median, 3), "min .. max": f"{min(ms):.3f} .. {max(ms):.3f}",
               "launches": summary["launches"], "tileVisits": summary["tileVisits"], "reached": reached, "seedsUsed": summary["seedsUsed"],
               "ms/Mreached": round(median / max(reached, 1) * 1e6, 3), "flag_ms": round(summary["launches"] * round_trip_ms, 3),
               "torch_ms": round(t_med, 2), "steps": steps, "torch / spread": round(t_med / median, 1), "same bytes": same,
               "working_MB": round(voxels * 2.125 / 1e6, 1), "pass_ms": round(t_med / max(steps, 1), 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    with open(out_path, "w") as fh:
        fh.write(f"# cvx_world_spread: tools/spread_bench.py {dim} {repeats}\n\n")
        fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}) on one MI355X; the box {list(lo)} .. {list(hi)} lies across the terrain's surface (y = {surface}) in the "
                 f"middle of the world; the pond's box ends at y = {surface + 1}.  The columns are explained at the top of tools/spread_bench.py; one 4-byte flag read "
                 f"measured {round_trip_ms:.4f} ms.  No threshold is set on any of these.\n\n")
        names = list(rows[0])
        fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
        for row in rows:
            fh.write("| " + " | ".join(str(row[n]) for n in names) + " |\n")


if __name__ == "__main__":
    main()
