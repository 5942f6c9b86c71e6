"""cvx_world_snapshot, cvx_world_snapshot_restore and cvx_world_snapshot_diff on the procedural world of bench.py, beside the path a restore
replaces: cvx_world_read_region of LOD 0 when the state is saved and cvx_world_edit of that blob when it is put back, in the same process and on
the same rectangles.
Usage: python tools/snapshot_bench.py [dim] [repeats] [out.md] ; prints one JSON line per rectangle and writes the tables to out.md (default
profiles/snapshot.md).

Per rectangle (64^2, 256^2 and 1024^2 columns in the middle of the world, levelCount 5), `repeats` rounds after one warm-up round; a round is
  save      snapshot = cvx_world_snapshot(rect, 5)            and, for the replaced path, blob = cvx_world_read_region(0, rect)
  edit      one cvx_world_brush call of 4096 spheres (FILL and CARVE in turn, radius 2 .. 5, across the terrain's surface inside the rectangle)
  diff      cvx_world_snapshot_diff_device into a torch tensor with room for every column, flags 0
  put back  cvx_world_snapshot_restore; then the same brush call again and cvx_world_edit(rect, blob, 5), the replaced path
and a check that both ways leave the same LOD 0 .. 5 over the rectangle (cvx_world_read_region, byte for byte).
Columns (milliseconds are medians over the rounds, `min .. max` beside the ones a claim rests on):
  capture_ms / capture_wall    the capture's own device time (outDeviceMs: events around everything it enqueues) / the host clock around the call
  MiB                          what the snapshot holds on the device (cvx_snapshot_info.deviceBytes); elements0 = the blob elements of LOD 0
  restore_ms / restore_wall    the same two clocks for the restore
  read_wall                    the host clock around cvx_world_read_region(0, rect): device work, the copy to the host, the malloc
  edit_ms / edit_wall          cvx_world_edit's device time (the upload of the blob included) / the host clock around it
  replaced_wall                read_wall + edit_wall, the wall time of the path a capture + restore replaces (capture_wall + restore_wall)
  diff_ms / diff_wall          the diff's two clocks; changed = the columns it lists; Mcol/s = the rectangle's columns per second of diff_ms
  diff_MB                      bytes the count pass reads, from the shapes: 16 per record and 12 per snapshot header and column, 4 per element of the
                               snapshot's LOD 0 and as many again for the arena's runs and colours; + 12 written per column; GB/s over diff_ms
  capture0_ms                  cvx_world_snapshot at levelCount 0: the read-back's count pass, scan and write pass over the same rectangle, the
                               nearest existing device work of the diff's shape that a host can time (the count pass alone: rocprofv3
                               --kernel-trace --stats in a run of its own, see the profile)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402


def clocked(call):
    """-> (what the call returns, wall milliseconds); every call here returns when the device is done."""
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1000.0


def spheres(rng, rect, surface, count=gpu.BRUSH_MAX_STROKES):
    x0, z0, sx, sz = rect
    out = np.zeros(count, dtype=gpu.STROKE_DTYPE)
    out["op"] = np.where(np.arange(count) % 2 == 0, gpu.BRUSH_FILL, gpu.BRUSH_CARVE)
    out["shape"] = gpu.SHAPE_SPHERE
    out["a"][:, 0] = rng.integers(x0 + 6, x0 + sx - 6, count)
    out["a"][:, 1] = surface + rng.integers(-8, 9, count)
    out["a"][:, 2] = rng.integers(z0 + 6, z0 + sz - 6, count)
    out["b"][:, 0] = rng.integers(2, 6, count)  # (a sphere's radius is b[0], strokes_array's convention)
    out["argb"] = 0xFF3060C0
    return out


def median(values):
    return float(np.median(values))


def span(values):
    return f"{min(values):.3f} .. {max(values):.3f}"


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "snapshot.md")
    t0 = time.perf_counter()
    ws = host.WorldSet.procedural(dim, dim, dim)
    dims = tuple(ws.dims)
    print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    cx, cz = dims[0] // 2, dims[2] // 2
    _, column = ctx.read_voxels((cx, 0, cz), (cx + 1, dims[1], cz + 1), want_argb=False)
    surface = int(np.nonzero(column[0, 0])[0].max()) + 1 if column.any() else dims[1] // 2
    rng = np.random.default_rng(7)
    region_levels = lambda rect: [ctx.read_region(k, *[v >> k for v in rect]) for k in range(6)]
    rows = []
    for side in (64, 256, 1024):
        if side > min(dims[0], dims[2]):
            continue
        rect = (cx - side // 2, cz - side // 2, side, side)
        n = side * side
        strokes = spheres(rng, rect, surface)
        listed = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        names = ("capture_ms", "capture_wall", "restore_ms", "restore_wall", "read_wall", "edit_ms", "edit_wall", "diff_ms", "diff_wall", "capture0_ms")
        t = {k: [] for k in names}
        same = True
        for round_ in range(repeats + 1):
            snapshot, capture_wall = clocked(lambda: ctx.world_snapshot(*rect, 5))
            capture_ms = snapshot.ms
            (blob, count), read_wall = clocked(lambda: ctx.read_region(0, *rect))
            with ctx.world_snapshot(*rect, 0) as flat:
                capture0_ms = flat.ms
            ctx.brush(strokes, 5)
            summary, diff_wall = clocked(lambda: snapshot.diff_device(listed.data_ptr(), n))
            diff_ms = snapshot.ms
            restore_ms, restore_wall = clocked(snapshot.restore)
            restored = region_levels(rect) if round_ == 0 else None
            ctx.brush(strokes, 5)
            edit_ms, edit_wall = clocked(lambda: ctx.edit(*rect, blob, count, 5))
            if round_ == 0:  # (the warm-up round, and the check that both ways leave the same levels)
                same = restored == region_levels(rect) and snapshot.diff(capacity=0)[1]["changedColumns"] == 0
            else:
                for k, v in zip(names, (capture_ms, capture_wall, restore_ms, restore_wall, read_wall, edit_ms, edit_wall, diff_ms, diff_wall, capture0_ms)):
                    t[k].append(v)
            info, changed = snapshot.info, summary["changedColumns"]
            snapshot.close()
            ctx.compact()  # (not timed: every round starts from an arena without the places the round before left behind)
        elements0 = (len(blob) - 12 * count) // 4
        diff_bytes = n * (16 + 12 + 12) + 2 * 4 * elements0
        m = {k: median(v) for k, v in t.items()}
        row = {"rect": f"{side} x {side}", "columns": n, "MiB": round(info["deviceBytes"] / 2**20, 2), "elements0": elements0,
               "capture_ms": round(m["capture_ms"], 3), "capture_wall": round(m["capture_wall"], 3),
               "restore_ms": round(m["restore_ms"], 3), "restore min .. max": span(t["restore_ms"]), "restore_wall": round(m["restore_wall"], 3),
               "read_wall": round(m["read_wall"], 3), "edit_ms": round(m["edit_ms"], 3), "edit min .. max": span(t["edit_ms"]), "edit_wall": round(m["edit_wall"], 3),
               "replaced_wall": round(m["read_wall"] + m["edit_wall"], 3), "snapshot_wall": round(m["capture_wall"] + m["restore_wall"], 3),
               "replaced / snapshot": round((m["read_wall"] + m["edit_wall"]) / (m["capture_wall"] + m["restore_wall"]), 2), "same levels": same,
               "changed": changed, "diff_ms": round(m["diff_ms"], 3), "diff min .. max": span(t["diff_ms"]), "diff_wall": round(m["diff_wall"], 3),
               "Mcol/s": round(n / m["diff_ms"] / 1e3, 1), "diff_MB": round(diff_bytes / 1e6, 2), "GB/s": round(diff_bytes / m["diff_ms"] / 1e6, 1),
               "capture0_ms": round(m["capture0_ms"], 3), "capture0 min .. max": span(t["capture0_ms"])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    tables = (("Capture and restore against cvx_world_read_region + cvx_world_edit",
               ("rect", "columns", "MiB", "elements0", "capture_ms", "capture_wall", "restore_ms", "restore min .. max", "restore_wall", "read_wall", "edit_ms",
                "edit min .. max", "edit_wall", "replaced_wall", "snapshot_wall", "replaced / snapshot", "same levels")),
              ("Diff after the 4096-sphere brush call",
               ("rect", "columns", "changed", "diff_ms", "diff min .. max", "diff_wall", "Mcol/s", "diff_MB", "GB/s", "capture0_ms", "capture0 min .. max")))
    with open(out_path, "w") as fh:
        fh.write(f"# cvx_world_snapshot: tools/snapshot_bench.py {dim} {repeats}\n\n")
        fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}) on one MI355X; the rectangles lie in the middle of the world, the spheres across the terrain's "
                 f"surface (y = {surface}); levelCount 5; medians of {repeats} rounds after a warm-up round.  The columns are explained at the top of "
                 f"tools/snapshot_bench.py.  No threshold is set on any of these.\n")
        for title, names in tables:
            fh.write(f"\n## {title}\n\n| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
            for row in rows:
                fh.write("| " + " | ".join(str(row[k]) for k in names) + " |\n")


if __name__ == "__main__":
    main()
