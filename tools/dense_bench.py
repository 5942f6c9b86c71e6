"""cvx_world_read_voxels / cvx_world_write_voxels on the procedural world of bench.py: a 64^3 box, a 256^3 box and a dimX x 64 x dimZ slab at the
terrain's surface, against the routes a host has without these calls.
Usage: python tools/dense_bench.py [dim] [repeats] [out.md] ; prints one JSON line per box and writes the tables to out.md (default
profiles/dense.md).  Every time is the median of `repeats` calls, two runs each (run 1 / run 2), in milliseconds.

Reads, per box:
  kernel_ms     cvx_world_read_voxels_device into torch tensors (both arrays), timed with events on the stream it is enqueued on; GB/s = the 5
                bytes stored per voxel over that time
  host_call_ms  cvx_world_read_voxels into host arrays, wall clock (kernel + the copy over PCIe)
  region_ms     the route that exists without the call: cvx_world_read_region of the footprint (wall clock) ...
  decode_ms     ... plus the decode of its RLE columns into the same dense arrays on the host (numpy, vectorised; asserted equal to the call's)
Writes, per box (COPY_REPLACE, LOD 0 + LOD 1..5; what is written is the box's own content shifted by three voxels, then the original again):
  device_ms     cvx_world_write_voxels_device from torch tensors: the call's own device time
  host_call_ms  cvx_world_write_voxels from host arrays, wall clock (the copy over PCIe included)
  brush_ms      a FILL box brush over the same box (cvx_world_brush's device time): the same rectangle through the same machinery with no
                dense data to read -- the comparison tools/brush_bench.py and cvx_world_copy used
  encode_ms / edit_ms   the route that exists without the call: WorldSet.from_voxels of the footprint's columns on the host (wall clock) and
                cvx_world_edit of its blob (wall clock); not measured for the slab (see profiles/dense.md)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X: 8 TB/s


def decode_region(blob, size_x, size_z, dim_y, y0, y1):
    """A sub-world blob (cvx_world_read_region / WorldSet.extract_region) -> (argb, solid) of shape (size_x, size_z, y1 - y0): what
    cvx_world_read_voxels gives for the footprint's box [y0, y1)."""
    n = size_x * size_z
    raw = np.frombuffer(blob, dtype=np.uint32)
    headers, pool = raw[:3 * n].reshape(n, 3).astype(np.int64), raw[3 * n:]
    off, run_count = headers[:, 0], headers[:, 1] & 0xFFFF
    first = np.cumsum(run_count) - run_count                       # the column's first run among all runs
    column = np.repeat(np.arange(n), run_count)
    k = np.arange(int(run_count.sum())) - first[column]            # the run's place in its column
    words = pool[off[column] + 1 + k].astype(np.int64)
    index, length = words & 0xFFFF, words >> 16
    below = np.cumsum(length) - length
    top = dim_y - (below - np.append(below, 0)[first][column])     # the run covers [top - length, top)
    keep = index != 0xFFFF
    column, index, length, top = column[keep], index[keep], length[keep], top[keep]
    colours = off[column] + run_count[column] + 2 + index          # the run's first colour (its top voxel's)
    run = np.repeat(np.arange(len(length)), length)
    j = np.arange(int(length.sum())) - (np.cumsum(length) - length)[run]
    y = top[run] - 1 - j
    inside = (y >= y0) & (y < y1)
    argb = np.zeros((n, y1 - y0), dtype=np.uint32)
    solid = np.zeros((n, y1 - y0), dtype=bool)
    argb[column[run][inside], y[inside] - y0] = pool[(colours[run] + j)[inside]]
    solid[column[run][inside], y[inside] - y0] = True
    return argb.reshape(size_x, size_z, y1 - y0), solid.reshape(size_x, size_z, y1 - y0)


def two_runs(call, repeats):
    """(median of run 1, median of run 2) of call() -> milliseconds."""
    return [round(float(np.median([call() for _ in range(repeats)])), 3) for _ in range(2)]


def wall(call):
    t = time.perf_counter()
    call()
    return (time.perf_counter() - t) * 1e3


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "dense.md")
    t0 = time.perf_counter()
    ws = host.WorldSet.procedural(dim, dim, dim)
    dims = tuple(ws.dims)
    print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    # the terrain's surface in the middle of the world: the boxes straddle it
    _, column = ctx.read_voxels((dims[0] // 2, 0, dims[2] // 2), (dims[0] // 2 + 1, dims[1], dims[2] // 2 + 1), want_argb=False)
    surface = int(np.nonzero(column[0, 0])[0].max()) + 1 if column.any() else dims[1] // 2

    def centred(size, height):
        lo = [dims[0] // 2 - size[0] // 2, max(0, min(dims[1] - height, surface - height // 2)), dims[2] // 2 - size[1] // 2]
        return tuple(lo), (lo[0] + size[0], lo[1] + height, lo[2] + size[1])

    side = min(256, dims[0])
    boxes = [("64^3", *centred((64, 64), 64)), (f"{side}^3", *centred((side, side), min(side, dims[1]))),
             (f"{dims[0]} x 64 x {dims[2]} slab", *centred((dims[0], dims[2]), 64))]
    stream = torch.cuda.Stream()  # (a stream of its own: torch's default stream has the handle 0, which the call reads as "the context's")
    ctx.brush([{"op": gpu.BRUSH_PAINT, "shape": gpu.SHAPE_BOX, "a": [0, 0, 0], "b": [1, 1, 1], "argb": 0xFF000000}], 5)  # (the first edit lays the arena out with headroom)
    reads, writes = [], []
    for name, lo, hi in boxes:
        shape = (hi[0] - lo[0], hi[2] - lo[2], hi[1] - lo[1])
        voxels = shape[0] * shape[1] * shape[2]
        slab = shape[0] * shape[1] > side * side
        d_argb = torch.empty(shape, dtype=torch.int32, device="cuda")
        d_solid = torch.empty(shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def read_kernel():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                a.record(stream)
                ctx.read_voxels_device(lo, hi, d_argb.data_ptr(), d_solid.data_ptr(), stream.cuda_stream)
                b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        read_kernel()  # (warm-up)
        kernel = two_runs(read_kernel, repeats)
        host_read = two_runs(lambda: wall(lambda: ctx.read_voxels(lo, hi)), 1 if slab else repeats)
        region = two_runs(lambda: wall(lambda: ctx.read_region(0, lo[0], lo[2], shape[0], shape[1])), 1 if slab else repeats)
        row = {"box": name, "min": list(lo), "voxels": voxels, "solid_fraction": round(float(d_solid.float().mean().item()), 3), "kernel_ms": kernel,
               "kernel_GBs": [round(5 * voxels / ms / 1e6, 1) for ms in kernel], "hbm_peak_GBs": HBM_PEAK_GBS, "host_call_ms": host_read, "region_ms": region}
        if slab:
            row["decode_ms"] = "not measured"
        else:
            blob, _ = ctx.read_region(0, lo[0], lo[2], shape[0], shape[1])
            row["decode_ms"] = two_runs(lambda: wall(lambda: decode_region(blob, shape[0], shape[1], dims[1], lo[1], hi[1])), repeats)
            argb, solid = decode_region(blob, shape[0], shape[1], dims[1], lo[1], hi[1])
            assert (argb.view(np.int32) == d_argb.cpu().numpy()).all() and (solid == d_solid.cpu().numpy().astype(bool)).all(), "the decoded region differs from the call's arrays"
        reads.append(row)
        print(json.dumps(row), flush=True)

        # writes: the content shifted by three voxels along x, then the original again
        original = (d_argb.clone(), d_solid.clone())
        shifted = (torch.roll(d_argb, 3, 0).contiguous(), torch.roll(d_solid, 3, 0).contiguous())
        torch.cuda.synchronize()
        state = [0]

        def write_device():
            a, s = (shifted, original)[state[0] % 2]
            state[0] += 1
            return ctx.write_voxels_device(lo, hi, a.data_ptr(), s.data_ptr(), gpu.COPY_REPLACE, 5)

        write_device(), write_device()  # (warm-up; the world is the original again)
        device = two_runs(write_device, repeats + repeats % 2)  # (an even count: the world ends as it was)
        row = {"box": name, "columns": shape[0] * shape[1], "device_ms": device}
        if not slab:
            h_shifted = (shifted[0].cpu().numpy().view(np.uint32), shifted[1].cpu().numpy())
            h_original = (original[0].cpu().numpy().view(np.uint32), original[1].cpu().numpy())

            def write_host():
                a, s = (h_shifted, h_original)[state[0] % 2]
                state[0] += 1
                return wall(lambda: ctx.write_voxels(lo, a, s, gpu.COPY_REPLACE, 5))

            row["host_call_ms"] = two_runs(write_host, repeats + repeats % 2)
            # without the call: the footprint's columns, whole, encoded on the host and pushed through cvx_world_edit
            a, s = ctx.read_voxels((lo[0], 0, lo[2]), (hi[0], dims[1], hi[2]))
            x, z, y = np.nonzero(s)
            colours = a[x, z, y]
            x, y, z = x.astype(np.int32), y.astype(np.int32), z.astype(np.int32)
            sub = [None]

            def encode():
                sub[0] = host.WorldSet.from_voxels((shape[0], dims[1], shape[1]), x, y, z, colours, threads=16)

            row["encode_ms"] = two_runs(lambda: wall(encode), repeats)
            blob, count = sub[0].extract_region(0, 0, 0, shape[0], shape[1])
            row["edit_ms"] = two_runs(lambda: wall(lambda: ctx.edit(lo[0], lo[2], shape[0], shape[1], blob, count, 5)), repeats)
        else:
            row["host_call_ms"] = row["encode_ms"] = row["edit_ms"] = "not measured"
        stroke = {"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": list(lo), "b": list(hi), "argb": 0xFF3070C0}
        ctx.brush([stroke], 5)  # (warm-up; from here on the box is one solid block: the brush re-emits the same columns every time)
        row["brush_ms"] = two_runs(lambda: ctx.brush([stroke], 5), repeats)
        ctx.write_voxels_device(lo, hi, original[0].data_ptr(), original[1].data_ptr(), gpu.COPY_REPLACE, 5)
        writes.append(row)
        print(json.dumps(row), flush=True)
        del d_argb, d_solid, original, shifted
        torch.cuda.empty_cache()
    used, abandoned, spare = ctx.edit_stats()
    ctx.close()

    def table(fh, rows):
        names = list(rows[0])
        fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
        for row in rows:
            fh.write("| " + " | ".join(" / ".join(str(x) for x in v) if isinstance(v, list) and names[i] != "min" else str(v)
                                       for i, v in enumerate(row[n] for n in names)) + " |\n")

    with open(out_path, "w") as fh:
        fh.write(f"# cvx_world_read_voxels, cvx_world_write_voxels: tools/dense_bench.py {dim} {repeats}\n\n")
        fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}), boxes centred on the terrain's surface (y = {surface}) in the middle of the world; medians of "
                 f"{repeats} calls, run 1 / run 2, milliseconds (see the tool's docstring for the columns).  Arena after the run: {used / 1e6:.1f} MB used, "
                 f"{abandoned / 1e6:.1f} MB left behind by edits.\n\n## Reads\n\n")
        table(fh, reads)
        fh.write("\n## Writes (COPY_REPLACE, LOD 0 + LOD 1..5)\n\n")
        table(fh, writes)


if __name__ == "__main__":
    main()
