"""cvx_world_lift_pieces on two scenes built on the device with brushes, beside today's route to the same arrays: per piece
cvx_world_spread_device through SOLID from the piece's seed, cvx_world_read_voxels_device of its bounding box and a torch mask, in the same
process on the same pieces.
Usage: python tools/lift_bench.py [repeats] [out.md] ; prints one JSON line per scene and writes the tables to out.md (default profiles/lift.md).

Scenes (a 256 x 64 x 256 world that holds a floor at y = 0):
  chunks    a 4-voxel slab over the whole world, 12 voxels above the floor, cut by carves into 32 x 32 = 1024 loose chunks of 7 x 4 x 7 voxels (6 along the far edges)
  lattice   ONE piece: a diagonal staircase of 60 overlapping 5 x 2 x 5 steps from one corner of the world towards the other, with a rung across
            every fourth step; its bounding box is mostly empty
Per scene, `repeats` rounds after one warm-up round; the floating pieces are those of anchors = GROUND over the whole world.
Columns (milliseconds are medians over the rounds with min .. max; `ms` is the call's own device time, outDeviceMs: events from the first enqueue of
the analysis to the last of the call; `wall` the host clock around the call, which returns when the device is done):
  report      cvx_world_lift_pieces_device, COPY, both capacities 0: the analysis and the total of the box volumes
  list        the same with a list capacity for every piece and no pools: + the nine sums per piece
  copy        COPY into torch tensors of neededVoxels elements: + the memsets and the write kernel
  remove      CVX_LIFT_REMOVE with the same pools: + the column edit over the stored pieces' rectangle at levelCount 5 (a cvx_world_snapshot of the
              whole world, taken outside the clock, puts the pieces back between rounds)
  pieces_rm   cvx_world_pieces with CVX_PIECES_REMOVE, the existing call that deletes the same voxels and hands nothing out
  route       cvx_world_pieces REPORT once, then per piece cvx_world_spread_device over its box from its seed (SPREAD_SOLID, every direction),
              cvx_world_read_voxels_device of the box and argb * (field >= 0), solid & (field >= 0) in torch; wall clock to a final
              torch.cuda.synchronize(), and `spread_ms` the sum of the spread calls' own device times.  The arrays are compared with the lift's,
              piece by piece, in the warm-up round.
  ratio       route wall / copy wall"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

DIMS = (256, 64, 256)
WHOLE = ((0, 0, 0), DIMS)
GROUND = gpu.ANCHOR_GROUND
FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE


def box(op, a, b, argb=0):
    return {"op": op, "shape": gpu.SHAPE_BOX, "a": a, "b": b, "argb": argb}


def chunks():
    strokes = [box(FILL, (0, 12, 0), (256, 16, 256), 0xFF8090A0)]
    for k in range(33):  # 33 cuts of one voxel each way, 8 apart: 32 x 32 chunks of 7 x 4 x 7
        at = min(8 * k, 255)
        strokes.append(box(CARVE, (at, 12, 0), (at + 1, 16, 256)))
        strokes.append(box(CARVE, (0, 12, at), (256, 16, at + 1)))
    return strokes


def lattice():
    strokes = []
    for k in range(60):
        x, y, z = 8 + 4 * k, 6 + 3 * k // 4, 8 + 4 * k
        strokes.append(box(FILL, (x, y, z), (x + 5, y + 2, z + 5), 0xFF406080 + k))
        if k % 4 == 0:
            strokes.append(box(FILL, (x, y, max(z - 12, 1)), (x + 1, y + 1, min(z + 17, 255)), 0xFFC04020))
    return strokes


def clocked(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1000.0


def stat(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def route(ctx, want=None):
    """Today's route -> (wall ms, summed spread device ms, pieces).  want: (lifted pieces, argb pool, solid pool) to compare with."""
    t0 = time.perf_counter()
    pieces, _, _ = ctx.world_pieces(*WHOLE, GROUND, gpu.PIECES_REPORT, capacity=1 << 16)
    spread_ms = 0.0
    kept = []
    for p in pieces:
        lo, hi = p["min"].tolist(), p["max"].tolist()
        n = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
        field = torch.empty(n, dtype=torch.int32, device="cuda")
        argb = torch.empty(n, dtype=torch.int32, device="cuda")
        solid = torch.empty(n, dtype=torch.uint8, device="cuda")
        _, ms = ctx.world_spread_device(lo, hi, [tuple(p["seed"].tolist())], field, medium=gpu.SPREAD_SOLID, max_steps=gpu.SPREAD_MAX_STEPS)
        spread_ms += ms
        ctx.read_voxels_device(lo, hi, argb.data_ptr(), solid.data_ptr())
        ctx.synchronize()  # (torch's stream is not the context's)
        own = field >= 0
        kept.append((argb * own, solid * own))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1000.0
    if want is not None:
        lifted, pool_argb, pool_solid = want
        assert len(lifted) == len(pieces)
        for k, (a, s) in enumerate(kept):
            at = int(lifted[k]["offset"])
            assert torch.equal(a, pool_argb[at:at + a.numel()]) and torch.equal(s, pool_solid[at:at + s.numel()]), f"piece {k}: the route and the lift differ"
    return wall, spread_ms, len(pieces)


def scene(name, strokes, repeats):
    solid = np.zeros(DIMS, dtype=bool)
    solid[:, 0, :] = True
    x, y, z = np.nonzero(solid)
    ws = host.WorldSet.from_voxels(DIMS, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), np.full(len(x), 0xFF305030, dtype=np.uint32), threads=8)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        ctx.brush(strokes, 5)
        none = torch.zeros(1, dtype=torch.uint8, device="cuda")  # (keeps torch's allocator warm before the first clocked call)
        del none
        _, totals, _ = ctx.world_lift_pieces_device(*WHOLE, GROUND, None, None, capacity=0)
        m, needed = totals["floatingPieces"], totals["neededVoxels"]
        argb = torch.zeros(needed, dtype=torch.int32, device="cuda")
        mask = torch.zeros(needed, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rows = {k: {"ms": [], "wall": []} for k in ("report", "list", "copy", "remove", "pieces_rm")}
        route_wall, route_spread = [], []
        with ctx.world_snapshot(0, 0, DIMS[0], DIMS[2], 5) as whole:
            for r in range(repeats + 1):
                calls = {
                    "report": lambda: ctx.world_lift_pieces_device(*WHOLE, GROUND, None, None, capacity=0),
                    "list": lambda: ctx.world_lift_pieces_device(*WHOLE, GROUND, None, None, capacity=m),
                    "copy": lambda: ctx.world_lift_pieces_device(*WHOLE, GROUND, argb, mask, capacity=m),
                    "remove": lambda: ctx.world_lift_pieces_device(*WHOLE, GROUND, argb, mask, gpu.LIFT_REMOVE, capacity=m),
                }
                for key, call in calls.items():
                    (pieces, got, ms), wall = clocked(call)
                    assert got["floatingPieces"] == m and got["neededVoxels"] == needed
                    if key == "remove":
                        assert got["storedPieces"] == m and ctx.world_pieces(*WHOLE, GROUND)[1]["floatingPieces"] == 0
                        whole.restore()
                    if r:
                        rows[key]["ms"].append(ms)
                        rows[key]["wall"].append(wall)
                (_, got, ms), wall = clocked(lambda: ctx.world_pieces(*WHOLE, GROUND, gpu.PIECES_REMOVE, capacity=0))
                whole.restore()
                if r:
                    rows["pieces_rm"]["ms"].append(ms)
                    rows["pieces_rm"]["wall"].append(wall)
                if r == 0 or r <= min(repeats, 3):  # (the route is slow: three clocked rounds at the most)
                    lifted, _, _ = ctx.world_lift_pieces_device(*WHOLE, GROUND, argb, mask, capacity=m)
                    wall, spread_ms, count = route(ctx, (lifted, argb, mask) if r == 0 else None)
                    assert count == m
                    if r:
                        route_wall.append(wall)
                        route_spread.append(spread_ms)
        voxels = int(ctx.world_pieces(*WHOLE, GROUND)[1]["floatingVoxels"])
        out = {"scene": name, "pieces": m, "voxels": voxels, "neededVoxels": needed, "repeats": repeats,
               **{k: {c: stat(v[c]) for c in ("ms", "wall")} for k, v in rows.items()},
               "route": {"wall": stat(route_wall), "spread_ms": stat(route_spread)}}
        out["ratio"] = out["route"]["wall"]["median"] / out["copy"]["wall"]["median"]
        return out
    finally:
        ctx.close()
        ws.close()


def cell(s):
    return f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lift.md")
    results = [scene("chunks", chunks(), repeats), scene("lattice", lattice(), repeats)]
    lines = ["# cvx_world_lift_pieces: device and wall milliseconds (tools/lift_bench.py)", "",
             f"{torch.cuda.get_device_name(0)}, world {DIMS[0]} x {DIMS[1]} x {DIMS[2]}, medians of {repeats} rounds after a warm-up round (min .. max).", "",
             "| scene | pieces | voxels | neededVoxels | call | device ms | wall ms |", "|---|---|---|---|---|---|---|"]
    for res in results:
        print(json.dumps(res))
        for key in ("report", "list", "copy", "remove", "pieces_rm"):
            lines.append(f"| {res['scene']} | {res['pieces']} | {res['voxels']} | {res['neededVoxels']} | {key} | {cell(res[key]['ms'])} | {cell(res[key]['wall'])} |")
        lines.append(f"| {res['scene']} | {res['pieces']} | {res['voxels']} | {res['neededVoxels']} | route | spread alone: {cell(res['route']['spread_ms'])} | "
                     f"{cell(res['route']['wall'])} |")
    lines += ["", "| scene | route wall / copy wall |", "|---|---|"] + [f"| {res['scene']} | {res['ratio']:.1f} |" for res in results]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
