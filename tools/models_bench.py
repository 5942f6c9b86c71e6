"""cvx_world_place_models / cvx_world_read_model on the procedural world of bench.py, against the dense calls that could do the axis-aligned part
of the job before.
Usage: python tools/models_bench.py [dim] [repeats] [out.md]   prints one JSON line per measurement and writes the table to out.md
                                                               (default profiles/models.md)
       python tools/models_bench.py [dim] --one identity|yaw|scatter|dense
                                                               warm-up, then ONE such call and nothing else: the run to put under a kernel
                                                               trace (rocprofv3 --kernel-trace --stats -- python tools/models_bench.py ...)
Every time is the median of `repeats` (at least 10) calls after a warm-up, in device milliseconds: the calls' own outDeviceMs, events on the
context's stream for the reads.  All edits are COPY_REPLACE with LOD 0 + LOD 1..5.

  (a) identity   one 256^3 model placed as it lies (cvx_world_place_models_device) against cvx_world_write_voxels_device of the same arrays and
                 box.  cvx_dense.hip is the parent commit's, unchanged: the library's write_voxels_device is the yardstick.
  (b) yaw        the same model turned 45 degrees about y, about its centre
  (c) scatter    1024 instances of a 32^3 model with random yaw and scale 0.75 .. 1.5 in ONE call, against 1024 write_voxels_device calls of 32^3
                 boxes at the same places (the sum of their device times)
  (d) read       cvx_world_read_model_device of 256^3 through the yaw's map against cvx_world_read_voxels_device of a 256^3 box"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

REPLACE = gpu.COPY_REPLACE


def median(call, repeats):
    return round(float(np.median([call() for _ in range(repeats)])), 3)


def about_centre(linear, size, centre):
    linear = np.asarray(linear, dtype=np.float64)
    return np.concatenate([linear, (np.asarray(centre, dtype=np.float64) - linear @ (np.asarray(size, dtype=np.float64) / 2))[:, None]], axis=1)


def yaw(degrees, scale=1.0):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return scale * np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def ball(n, device):
    """A generated n^3 model on the device, (X, Z, Y): a ball with a colour per voxel, as int32 colour words."""
    x, z, y = torch.meshgrid(*[torch.arange(n, device=device)] * 3, indexing="ij")
    inside = (x - n / 2) ** 2 + (y - n / 2) ** 2 + (z - n / 2) ** 2 < (n / 2) ** 2
    words = 0xFF000000 + ((x * 5 + y * 3 + z * 7) & 0xFF) * 0x010101
    return torch.where(inside, words - (1 << 32), torch.zeros_like(words)).to(torch.int32).contiguous()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    one = None
    if "--one" in sys.argv:
        one = sys.argv[sys.argv.index("--one") + 1]
        args.remove(one)
    dim = int(args[0]) if len(args) > 0 else 2048
    repeats = max(10, int(args[1])) if len(args) > 1 else 10
    out_path = args[2] if len(args) > 2 else os.path.join(ROOT, "profiles", "models.md")
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
        big, small = min(256, dim // 2), 32
        model, prefab = ball(big, "cuda"), ball(small, "cuda")
        stream.synchronize()
        centre = (dims[0] / 2, dims[1] / 2, dims[2] / 2)
        lo = tuple(int(c - big / 2) for c in centre)
        hi = tuple(v + big for v in lo)
        size = (big, big, big)
        identity = gpu.model_instance(about_centre(np.eye(3), size, centre), size, 0, REPLACE)
        for a in range(3):  # (the dense write's box exactly)
            identity.boxMin[a], identity.boxMax[a] = lo[a], hi[a]
        turned = gpu.model_instance(about_centre(yaw(45), size, centre), size, 0, REPLACE)
        rng = np.random.default_rng(1)
        places = [(int(rng.integers(64, dims[0] - 64)), int(dims[1] * 0.75) + int(rng.integers(-32, 32)), int(rng.integers(64, dims[2] - 64))) for _ in range(1024)]
        scatter = [gpu.model_instance(about_centre(yaw(float(rng.uniform(0, 360)), float(rng.uniform(0.75, 1.5))), (small,) * 3, p), (small,) * 3, 0, REPLACE)
                   for p in places]
        calls = {
            "identity": lambda: ctx.place_models_device([(size, model.data_ptr(), 0)], [identity], 5),
            "yaw": lambda: ctx.place_models_device([(size, model.data_ptr(), 0)], [turned], 5),
            "scatter": lambda: ctx.place_models_device([((small,) * 3, prefab.data_ptr(), 0)], scatter, 5),
            "dense": lambda: ctx.write_voxels_device(lo, hi, model.data_ptr(), 0, REPLACE, 5),
        }
        if one:
            calls[one](), calls[one]()
            print(json.dumps({"one": one, "device_ms": round(calls[one](), 3)}), flush=True)
            ctx.set_stream(None)
            ctx.close()
            return

        # (a)
        calls["dense"](), calls["dense"]()
        dense_ms = median(calls["dense"], repeats)
        after_dense = ctx.read_region(0, lo[0], lo[2], big, big)[0]
        calls["identity"](), calls["identity"]()
        identity_ms = median(calls["identity"], repeats)
        assert ctx.read_region(0, lo[0], lo[2], big, big)[0] == after_dense, "the identity placement and the dense write leave different columns"
        report({"what": f"(a) write_voxels_device, {big}^3 box", "voxels": big ** 3, "device_ms": dense_ms})
        report({"what": f"(a) place_models_device, the same {big}^3 model at the identity", "voxels": big ** 3, "device_ms": identity_ms, "ratio": round(identity_ms / dense_ms, 3)})
        # (b)
        calls["yaw"](), calls["yaw"]()
        yaw_ms = median(calls["yaw"], repeats)
        report({"what": f"(b) place_models_device, the {big}^3 model at 45 degrees yaw", "columns": (turned.boxMax[0] - turned.boxMin[0]) * (turned.boxMax[2] - turned.boxMin[2]),
                "device_ms": yaw_ms, "ratio": round(yaw_ms / dense_ms, 3)})
        ctx.compact()
        # (c)
        def dense_scatter():
            return sum(ctx.write_voxels_device((p[0] - 16, p[1] - 16, p[2] - 16), (p[0] + 16, p[1] + 16, p[2] + 16), prefab.data_ptr(), 0, REPLACE, 5) for p in places)

        dense_scatter()
        many_ms = median(dense_scatter, 3)
        ctx.compact()
        calls["scatter"](), calls["scatter"]()
        scatter_ms = median(calls["scatter"], repeats)
        report({"what": "(c) 1024 write_voxels_device calls of 32^3 boxes (sum of their device ms)", "device_ms": many_ms})
        report({"what": "(c) place_models_device, 1024 instances of a 32^3 model, random yaw and scale, one call", "device_ms": scatter_ms, "ratio": round(scatter_ms / many_ms, 3)})
        ctx.compact()
        # (d)
        out_argb = torch.empty(big ** 3, dtype=torch.int32, device="cuda")
        out_mask = torch.empty(big ** 3, dtype=torch.uint8, device="cuda")
        inverse = np.linalg.inv(np.vstack([about_centre(yaw(45), size, centre), [0, 0, 0, 1]]))[:3]
        to_world = gpu.model_instance(inverse, dims).toModel

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            stream.synchronize()
            return a.elapsed_time(b)

        read_box = lambda: timed(lambda: ctx.read_voxels_device(lo, hi, out_argb.data_ptr(), out_mask.data_ptr()))  # noqa: E731
        read_model = lambda: timed(lambda: ctx.read_model_device(size, to_world, out_argb.data_ptr(), out_mask.data_ptr()))  # noqa: E731
        read_box(), read_model()
        box_ms, model_ms = median(read_box, repeats), median(read_model, repeats)
        report({"what": f"(d) read_voxels_device, {big}^3 box", "voxels": big ** 3, "device_ms": box_ms, "GBs": round(5 * big ** 3 / box_ms / 1e6, 1)})
        report({"what": f"(d) read_model_device, {big}^3 at 45 degrees yaw", "voxels": big ** 3, "device_ms": model_ms, "GBs": round(5 * big ** 3 / model_ms / 1e6, 1),
                "ratio": round(model_ms / box_ms, 3)})
    used, abandoned, _ = ctx.edit_stats()
    ctx.set_stream(None)
    ctx.close()
    with open(out_path, "w") as fh:
        fh.write(f"# cvx_world_place_models, cvx_world_read_model: tools/models_bench.py {dim} {repeats}\n\n")
        fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}); medians of {repeats} calls after warm-up, device milliseconds (see the tool's docstring).  "
                 f"Arena after the run: {used / 1e6:.1f} MB used, {abandoned / 1e6:.1f} MB left behind by edits.\n\n")
        names = ["what", "columns", "voxels", "device_ms", "GBs", "ratio"]
        fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
        for row in rows:
            fh.write("| " + " | ".join(str(row.get(n, "")) for n in names) + " |\n")


if __name__ == "__main__":
    main()
