"""cvxv_models_draw_device on bodies lifted from the procedural world of bench.py, drawn into the blitted frame of that world, beside the two routes
a host has without the call.
Usage: python tools/model_draw_bench.py [dim] [repeats] [out.md] [width] [height] ; prints one JSON line per case and writes the table to out.md
(default profiles/model_draw.md; whatever follows a line "## Kernel resources" in an existing file is kept).

Bodies: tools/model_pick_bench.py's -- tools/contacts_bench.py's loose chunks of 7 x 4 x 7 voxels, lifted with cvx_world_lift_pieces_device into torch
pools, piled up as tools/pair_contacts_bench.py piles them, each under a yaw and a tilt of its own -- 1, 64 and 1024 of them.  The eye stands 60
voxels above the terrain at (dim / 2, dim * 0.3), pitched 20 degrees down; the pile stands before it at 60 % of the distance to the terrain along
the middle pixel's ray (120 voxels at the most).  The frame is width x height (default 1920 x 1080); the call writes colour into the image cvx_blit_segments left on the device, and depth and
ids into torch tensors.
Columns (milliseconds are medians over `repeats` rounds after a warm-up round, with min .. max):
  jobs, drawn, occluded    the call's summary
  draw                     this call without and with CVXV_DRAW_WORLD: its own device time (outDeviceMs) / the host clock around it
  (A) place route          what the documented route costs ON TOP of the frame: cvx_world_snapshot of the pile's footprint, cvx_world_place_models_device
                           (FILL, all LODs), restore -- the sum of the three calls' device times / the host clock around them
  (B) pick route           the same rays (cvxv_view_rays, uploaded once, not timed) through cvxq_model_pick_device and cvx_world_pick_device in chunks
                           of 65 536: the model picks' device times summed / the host clock around all of it; its instances are compared with the ids"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from contacts_bench import CORNER, cell, chunk_strokes, rotation, stat  # noqa: E402

FILL = gpu.BRUSH_FILL
MARKER = "## Kernel resources"
BODIES = (1, 64, 1024)
CHUNK = gpu.MODEL_PICK_MAX_RAYS


def pile_at(count, sizes, rng, centre):
    """tools/pair_contacts_bench.py's pile, its middle at `centre`."""
    side = int(np.ceil(count ** (1 / 3)))
    middle = np.array([3.0 * (side - 1), 1.5 * (side - 1), 3.0 * (side - 1)])
    instances = []
    for k in range(count):
        size = sizes[k % len(sizes)]
        gx, gz, gy = k % side, (k // side) % side, k // (side * side)
        at = np.asarray(centre, dtype=np.float64) - middle + np.array([6 * gx, 3 * gy, 6 * gz], dtype=np.float64) + rng.uniform(-1, 1, 3)
        linear = rotation(1, float(rng.uniform(0, 360))) @ rotation(0, float(rng.uniform(-20, 20)))
        forward = np.concatenate([linear, (at - linear @ (np.asarray(size, dtype=np.float64) / 2))[:, None]], axis=1)
        instances.append(gpu.model_instance(forward, size, k % len(sizes), FILL))
    return instances


def timed(repeats, call):
    """call() -> device ms, or (device ms, wall ms) where it takes the host clock itself; (device stat, wall stat) over `repeats` rounds after a
    warm-up round."""
    device_ms, wall_ms = [], []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        ms = call()
        wall = (time.perf_counter() - t0) * 1000.0
        if isinstance(ms, tuple):
            ms, wall = ms
        if r:
            device_ms.append(ms)
            wall_ms.append(wall)
    return stat(device_ms), stat(wall_ms)


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "model_draw.md")
    width = int(sys.argv[4]) if len(sys.argv) > 4 else 1920
    height = int(sys.argv[5]) if len(sys.argv) > 5 else 1080
    ws = host.WorldSet.procedural(dim, dim, dim)
    ctx = gpu.Context(0)
    rows = []
    try:
        ctx.upload_world(ws)
        ctx.set_resolution(width, height)
        y0 = dim - 64
        ctx.brush(chunk_strokes(y0), 5)
        lift_box = ((0, y0 - 1, 0), (CORNER, y0 + 5, CORNER))
        _, totals, _ = ctx.world_lift_pieces_device(*lift_box, gpu.ANCHOR_GROUND, None, None, capacity=0)
        argb = torch.zeros(totals["neededVoxels"], dtype=torch.int32, device="cuda")
        mask = torch.zeros(totals["neededVoxels"], dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pieces, totals, _ = ctx.world_lift_pieces_device(*lift_box, gpu.ANCHOR_GROUND, argb, mask, gpu.LIFT_REMOVE, capacity=1024)
        assert totals["storedPieces"] == 1024 == len(pieces)
        device_models = [gpu.lifted_model(pieces, k, argb.data_ptr(), mask.data_ptr()) for k in range(gpu.MODELS_MAX_MODELS)]

        # the frame of the world: rendered and blitted once, the image stays on the device
        # (the benchmark path flies outside the world, where nothing can be placed: the eye stands 60 voxels above the terrain inside it)
        _, _, _, down = ctx.pick([(0.5 * dim, dim + 8.0, 0.3 * dim)], [(0.0, -1.0, 0.0)], 1e4)
        position, euler = [0.5 * dim, dim + 8.0 - float(down[0]) + 60.0, 0.3 * dim], (20.0, 30.0, 0.0)
        pose = host.camera_pose(position, euler, width, height)
        lods, far = host.setup_lods(pose, ws.max_dimension, width, height, 1.0)
        frame = host.setup_frame(pose, lods, far, width, height, ws.dims[1], True)
        ctx.draw_segments(frame, 0)
        ctx.blit_segments(0, to_host=False)
        image_ptr, _ = ctx.screen_device_ptr()
        view = gpu.view_from_camera(frame.camera, width, height, 1e4)
        middle = gpu.view_rays(view, width // 2, height // 2, 1, 1)[0, 0]
        _, face, _, t = ctx.pick(middle["origin"][None], middle["direction"][None], 1e4)
        distance = min(120.0, 0.6 * float(t[0])) if face[0] >= 0 else 120.0
        centre = middle["origin"].astype(np.float64) + distance * middle["direction"].astype(np.float64)

        pixels = width * height
        depth_t = torch.empty(pixels, dtype=torch.float32, device="cuda")
        ids_t = torch.empty(pixels, dtype=torch.int32, device="cuda")
        rays_t = torch.from_numpy(gpu.view_rays(view).reshape(-1).view(np.uint8).copy()).cuda()
        hits_t = torch.zeros(pixels * 48, dtype=torch.uint8, device="cuda")
        picks_t = torch.zeros(CHUNK * 24, dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()  # (torch's default stream has the handle 0, which cvx_world_pick_device reads as "the context's")
        rng = np.random.default_rng(1080)
        for bodies in BODIES:
            instances = pile_at(bodies, [m[0] for m in device_models], rng, centre)
            models = device_models[:min(bodies, len(device_models))]
            lo = np.min([list(i.boxMin) for i in instances], axis=0)
            hi = np.max([list(i.boxMax) for i in instances], axis=0)
            row = {"bodies": bodies, "distance": round(distance, 1)}

            def draw(flags):
                depth_t.fill_(float("inf"))
                ids_t.fill_(-1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                summary, ms = ctx.models_draw_device(models, instances, view, flags, image_ptr, depth_t, ids_t)
                wall = (time.perf_counter() - t0) * 1000.0
                row.update(summary if flags else {"jobs": summary["jobs"]})
                return ms, wall
            row["draw_ms"], row["draw_wall_ms"] = timed(repeats, lambda: draw(0))
            plain_ids = ids_t.cpu().numpy().copy()
            row["draw_world_ms"], row["draw_world_wall_ms"] = timed(repeats, lambda: draw(gpu.DRAW_WORLD))

            def place_route():
                snapshot = ctx.world_snapshot(int(lo[0]), int(lo[2]), int(hi[0] - lo[0]), int(hi[2] - lo[2]), 5)
                ms = snapshot.ms + ctx.place_models_device(models, instances, 5)  # (the frame would be drawn here)
                ms += snapshot.restore()
                snapshot.close()
                return ms
            row["place_ms"], row["place_wall_ms"] = timed(repeats, place_route)

            def pick_route():
                total = 0.0
                for first in range(0, pixels, CHUNK):
                    n = min(CHUNK, pixels - first)
                    total += ctx.model_pick_device(models, instances, rays_t[first * 32:(first + n) * 32], hits_t[first * 48:(first + n) * 48], n)
                    assert gpu.lib().cvx_world_pick_device(ctx._h, n, C.c_void_p(rays_t.data_ptr() + first * 32), C.c_void_p(picks_t.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
                side.synchronize()
                return total
            row["pick_ms"], row["pick_wall_ms"] = timed(min(repeats, 3), pick_route)
            picked = hits_t.cpu().numpy().view(gpu.MODEL_HIT_DTYPE)["instance"]
            row["ids_equal_picks"] = bool((picked == plain_ids).all())
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        ctx.close()
        ws.close()
    lines = ["# cvxv_models_draw: device / wall milliseconds beside the place route and the pick route (tools/model_draw_bench.py)", "",
             f"{torch.cuda.get_device_name(0)}, procedural world {dim}^3, frame {width} x {height} from 60 voxels above the terrain, the pile {rows[0]['distance']} voxels "
             f"before the eye; medians of {repeats} rounds after a warm-up round (min .. max), the pick route over {min(repeats, 3)} rounds.", "",
             "| bodies | jobs | drawn | occluded | draw device ms | draw wall ms | draw + world device ms | draw + world wall ms | (A) place route device ms | (A) wall ms | "
             "(B) pick route model-pick device ms | (B) wall ms | ids = (B)'s instances |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        lines.append(f"| {row['bodies']} | {row['jobs']} | {row['pixelsDrawn']} | {row['pixelsOccluded']} | {cell(row['draw_ms'])} | {cell(row['draw_wall_ms'])} | "
                     f"{cell(row['draw_world_ms'])} | {cell(row['draw_world_wall_ms'])} | {cell(row['place_ms'])} | {cell(row['place_wall_ms'])} | {cell(row['pick_ms'])} | "
                     f"{cell(row['pick_wall_ms'])} | {row['ids_equal_picks']} |")
    lines.append("")
    kept = ""
    if os.path.exists(out_path):
        text = open(out_path).read()
        kept = text[text.index(MARKER):] if MARKER in text else ""
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
