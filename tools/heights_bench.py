"""cvx_world_read_heights / cvx_world_write_heights on the procedural world of bench.py, against the two ways the same edit could be made before.
Usage: python tools/heights_bench.py [dim] [repeats] [out.md]   prints one JSON line per measurement and writes the tables to out.md
                                                                (default profiles/heights.md)
       python tools/heights_bench.py [dim] --one-write          warm-up, then ONE whole-footprint write and nothing else: the run to put under a
                                                                kernel trace (rocprofv3 --kernel-trace --stats -- python tools/heights_bench.py ...)
       python tools/heights_bench.py [dim] --one-tile-write     the same with the 256 x 256 tile
Every time is the median of `repeats` (at least 20) calls after a warm-up, in device milliseconds: the calls' own outDeviceMs, events on the
context's stream for the read.

  read            cvx_world_read_heights_device of the whole footprint, window [0, dimY), all three arrays; GB/s = the 12 bytes stored per column
  write whole     cvx_world_write_heights_device, COPY_REPLACE, thickness 2, LOD 0 + LOD 1..5, the whole footprint; the heights are the read-back
                  heights plus a smooth bump, then the read-back heights again, in turn
  write tile      the same over a 256 x 256 tile in the middle of the world
  (a) dense       cvx_world_write_voxels_device of the pre-expanded arrays (the expansion is made with torch on the device and not timed) over a
                  box of 512 x dimY x 512 voxels, and cvx_world_write_heights_device of the same box with the same heights
  (b) brush       a flat height field over the tile: cvx_world_write_heights_device (REPLACE, thickness t, one colour) against cvx_world_brush with
                  the two box strokes that make it (CARVE the window, FILL the slab); the tile reads back the same after either"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s
REPLACE = gpu.COPY_REPLACE


def median(call, repeats):
    return round(float(np.median([call() for _ in range(repeats)])), 3)


def expand(heights, argb, y0, y1, thickness):
    """The dense (X, Z, Y) arrays of the contract for a write without sideArgb and without WALLED, on the device: (argb int32, solid uint8)."""
    H = heights.clamp(y0, y1)
    pad = torch.nn.functional.pad(H[None, None].float(), (1, 1, 1, 1), mode="replicate")[0, 0].to(torch.int32)
    low = torch.minimum(torch.minimum(pad[:-2, 1:-1], pad[2:, 1:-1]), torch.minimum(pad[1:-1, :-2], pad[1:-1, 2:]))
    b = (torch.minimum(H, low) - thickness).clamp(min=y0) if thickness else torch.full_like(H, y0)
    y = torch.arange(y0, y1, dtype=torch.int32, device=heights.device)[None, None, :]
    solid = (b[:, :, None] <= y) & (y < H[:, :, None])
    colours = torch.where(solid, argb[:, :, None], torch.zeros((), dtype=torch.int32, device=heights.device)).contiguous()
    return colours, solid.to(torch.uint8).contiguous()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    one_write, one_tile_write = "--one-write" in sys.argv, "--one-tile-write" in sys.argv
    dim = int(args[0]) if len(args) > 0 else 2048
    repeats = max(20, int(args[1])) if len(args) > 1 else 20
    out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "heights.md")
    ws = host.WorldSet.procedural(dim, dim, dim)
    dims = tuple(ws.dims)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    stream = torch.cuda.Stream()  # the context's stream from here on: torch's work on the arrays and the calls are ordered on it
    ctx.set_stream(stream.cuda_stream)
    ctx.brush([{"op": gpu.BRUSH_PAINT, "shape": gpu.SHAPE_BOX, "a": [0, 0, 0], "b": [1, 1, 1], "argb": 0xFF000000}], 5)  # (the first edit lays the arena out with headroom)
    rows = []

    def report(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    with torch.cuda.stream(stream):
        whole = ((0, 0, 0), dims)
        shape = (dims[0], dims[2])
        heights = torch.empty(shape, dtype=torch.int32, device="cuda")
        argb = torch.empty(shape, dtype=torch.int32, device="cuda")
        bottoms = torch.empty(shape, dtype=torch.int32, device="cuda")

        def read():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctx.read_heights_device(*whole, heights.data_ptr(), argb.data_ptr(), bottoms.data_ptr())
            b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        read()
        xs, zs = torch.meshgrid(torch.arange(shape[0], device="cuda"), torch.arange(shape[1], device="cuda"), indexing="ij")
        bump = (24 * torch.exp(-((xs - shape[0] / 2) ** 2 + (zs - shape[1] / 2) ** 2) / (2 * (min(shape) / 6.0) ** 2))).to(torch.int32)
        raised = (heights + bump).clamp(max=dims[1]).contiguous()
        stream.synchronize()
        state = [0]

        def write(lo, hi, pair, colours, thickness=2):
            h = pair[state[0] % 2]
            state[0] += 1
            return ctx.write_heights_device(lo, hi, h.data_ptr(), colours.data_ptr(), 0, thickness, 0, REPLACE, 5)

        write(*whole, (raised, heights), argb), write(*whole, (raised, heights), argb)  # (warm-up; the ground is the read-back heights' crust again)
        if one_write:
            ms = write(*whole, (raised, heights), argb)
            print(json.dumps({"one_write_ms": round(ms, 3), "columns": shape[0] * shape[1]}), flush=True)
            ctx.set_stream(None)
            ctx.close()
            return
        ms = 0.0 if one_tile_write else median(read, repeats)
        if not one_tile_write:
            report({"what": "read, whole footprint", "columns": shape[0] * shape[1], "device_ms": ms, "GBs": round(12 * shape[0] * shape[1] / ms / 1e6, 1), "hbm_peak_GBs": HBM_PEAK_GBS})
        report({"what": "write whole footprint (REPLACE, thickness 2)", "columns": shape[0] * shape[1], "device_ms": median(lambda: write(*whole, (raised, heights), argb), repeats)})

        ctx.compact()  # (every whole-footprint write leaves the columns it replaced behind: reclaim them before the smaller boxes)

        def sub(size):
            x0, z0 = (dims[0] - size) // 2, (dims[2] - size) // 2
            cut = lambda t: t[x0:x0 + size, z0:z0 + size].contiguous()  # noqa: E731
            return (x0, 0, z0), (x0 + size, dims[1], z0 + size), (cut(raised), cut(heights)), cut(argb)

        side = min(256, dims[0])
        lo, hi, pair, colours = sub(side)
        write(lo, hi, pair, colours), write(lo, hi, pair, colours)
        if one_tile_write:
            print(json.dumps({"one_tile_write_ms": round(write(lo, hi, pair, colours), 3), "columns": side * side}), flush=True)
            ctx.set_stream(None)
            ctx.close()
            return
        report({"what": f"write {side} x {side} tile (REPLACE, thickness 2)", "columns": side * side, "device_ms": median(lambda: write(lo, hi, pair, colours), repeats)})

        # (a) the dense write of the expansion, over the largest box it takes comfortably, against the heights write of the same box
        big = min(512, dims[0])
        lo, hi, pair, colours = sub(big)
        dense = [expand(h, colours, 0, dims[1], 2) for h in pair]
        stream.synchronize()

        def write_dense():
            a, s = dense[state[0] % 2]
            state[0] += 1
            return ctx.write_voxels_device(lo, hi, a.data_ptr(), s.data_ptr(), REPLACE, 5)

        write_dense(), write_dense()
        dense_ms = median(write_dense, repeats)
        after_dense = ctx.read_region(0, lo[0], lo[2], big, big)[0]
        write(lo, hi, pair, colours), write(lo, hi, pair, colours)
        heights_ms = median(lambda: write(lo, hi, pair, colours), repeats)
        assert ctx.read_region(0, lo[0], lo[2], big, big)[0] == after_dense, "the heights write and the dense write of its expansion leave different columns"
        report({"what": f"(a) {big} x {dims[1]} x {big} box: write_voxels_device of the expansion", "voxels": big * big * dims[1], "array_bytes": 5 * big * big * dims[1], "device_ms": dense_ms})
        report({"what": f"(a) the same box: write_heights_device", "columns": big * big, "array_bytes": 8 * big * big, "device_ms": heights_ms,
                "ratio_to_dense": round(heights_ms / dense_ms, 3)})
        del dense
        torch.cuda.empty_cache()
        ctx.compact()

        # (b) a flat field over the tile against the two box strokes that make it
        lo, hi, pair, colours = sub(side)
        level, t, colour = int(heights.float().mean().item()), 4, 0xFF40A060
        flat = torch.full((side, side), level, dtype=torch.int32, device="cuda")
        one = torch.full((side, side), colour - (1 << 32), dtype=torch.int32, device="cuda")
        stream.synchronize()
        strokes = [{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_BOX, "a": list(lo), "b": list(hi), "argb": 0},
                   {"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": [lo[0], level - t, lo[2]], "b": [hi[0], level, hi[2]], "argb": colour}]
        ctx.brush(strokes, 5)
        after_brush = ctx.read_region(0, lo[0], lo[2], side, side)[0]
        brush_ms = median(lambda: ctx.brush(strokes, 5), repeats)
        write(lo, hi, (flat, flat), one, t)
        assert ctx.read_region(0, lo[0], lo[2], side, side)[0] == after_brush, "the flat field and the two strokes leave different columns"
        flat_ms = median(lambda: write(lo, hi, (flat, flat), one, t), repeats)
        report({"what": f"(b) flat field over the {side} x {side} tile: write_heights_device", "device_ms": flat_ms})
        report({"what": "(b) the same: cvx_world_brush, CARVE the window + FILL the slab", "device_ms": brush_ms, "heights_to_brush": round(flat_ms / brush_ms, 3)})
    used, abandoned, _ = ctx.edit_stats()
    ctx.set_stream(None)
    ctx.close()
    with open(out_path, "w") as fh:
        fh.write(f"# cvx_world_read_heights, cvx_world_write_heights: tools/heights_bench.py {dim} {repeats}\n\n")
        fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}); medians of {repeats} calls after warm-up, device milliseconds (see the tool's docstring).  "
                 f"Arena after the run: {used / 1e6:.1f} MB used, {abandoned / 1e6:.1f} MB left behind by edits.\n\n")
        names = ["what", "columns", "voxels", "array_bytes", "device_ms", "GBs", "ratio_to_dense", "heights_to_brush"]
        fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
        for row in rows:
            fh.write("| " + " | ".join(str(row.get(n, "")) for n in names) + " |\n")


if __name__ == "__main__":
    main()
