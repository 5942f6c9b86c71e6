"""cvxq_model_pick_device on bodies lifted from the procedural world of bench.py, beside the only route a host has without the call -- FILL every
body into an empty scratch world with cvx_world_place_models_device, cvx_world_pick_device, CARVE them out again -- and beside a lane-per-job
build of the same rule.
Usage: python tools/model_pick_bench.py [dim] [repeats] [out.md] ; prints one JSON line per case and writes the table to out.md (default
profiles/model_pick.md; whatever follows a line "## Kernel resources" in an existing file is kept).

Bodies: tools/pair_contacts_bench.py's pile of tools/contacts_bench.py's loose chunks of 7 x 4 x 7 voxels, lifted with
cvx_world_lift_pieces_device into torch pools, each under a yaw and a tilt of its own.  Rays: from a sphere around the pile towards random points of
it, maxT 1e4.  Cases: 1, 64 and 4096 rays against 1, 64 and 1024 bodies.
Columns (milliseconds are medians over `repeats` rounds after a warm-up round, with min .. max):
  jobs        the (ray, instance) pairs whose box the ray crosses (counted here with the slab test in numpy)
  device ms   the call's own device time (outDeviceMs); wall ms: the host clock around the call, which returns when the hits are complete
  route ms    the host clock around FILL of all bodies, cvx_world_pick_device and its synchronisation, CARVE of all bodies; `same`: the share of rays
              on which the route names the call's voxel (where bodies overlap, the stamp's last writer is not the ray's nearest body)
  lane ms     device ms of the same call in the lane-per-job build, when cpuvox_amd/libcpuvox_gpu_lanepick.so exists
              (make -C cpuvox_amd/csrc variant NAME=lanepick DEFS=-DCVXQ_LANE_PER_JOB); its hits are compared with the product's byte for byte"""
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
from contacts_bench import CORNER, cell, chunk_strokes, stat  # noqa: E402
from pair_contacts_bench import SCRATCH, pile  # noqa: E402

FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE
MARKER = "## Kernel resources"
VARIANT = os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu_lanepick.so")
BODIES, RAYS = (1, 64, 1024), (1, 64, 4096)


def rays_at(instances, count, rng):
    lo = np.min([list(i.boxMin) for i in instances], axis=0).astype(np.float64)
    hi = np.max([list(i.boxMax) for i in instances], axis=0).astype(np.float64)
    centre, radius = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2 + 8
    away = rng.normal(size=(count, 3))
    o = centre + radius * away / np.linalg.norm(away, axis=1, keepdims=True)
    rays = np.zeros(count, dtype=gpu.PICK_RAY_DTYPE)
    rays["origin"], rays["direction"], rays["maxT"] = o, lo + rng.uniform(0, 1, size=(count, 3)) * (hi - lo) - o, 1e4
    return rays


def count_jobs(instances, rays):
    """The pairs whose box the ray crosses: the slab test of the pair rule, in float64."""
    o, d = rays["origin"].astype(np.float64)[:, None, :], rays["direction"].astype(np.float64)[:, None, :]
    lo = np.array([list(i.boxMin) for i in instances], dtype=np.float64)[None]
    hi = np.array([list(i.boxMax) for i in instances], dtype=np.float64)[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    enter, leave = np.minimum(t0, t1).max(axis=2), np.maximum(t0, t1).min(axis=2)
    return int((np.maximum(enter, 0.0) <= np.minimum(leave, rays["maxT"][:, None])).sum())


def timed_calls(ctx, models, instances, rays_t, hits_t, repeats):
    device_ms, wall_ms = [], []
    for r in range(repeats + 1):
        t0 = time.perf_counter()
        ms = ctx.model_pick_device(models, instances, rays_t, hits_t)
        wall = (time.perf_counter() - t0) * 1000.0
        if r:
            device_ms.append(ms)
            wall_ms.append(wall)
    return stat(device_ms), stat(wall_ms), hits_t.cpu().numpy().view(gpu.MODEL_HIT_DTYPE).copy()


def route(scratch, models, instances, rays_t, picks_t, side):
    """FILL all, pick, CARVE all -> the picks."""
    scratch.place_models_device(models, [with_op(i, FILL) for i in instances], 0)
    assert gpu.lib().cvx_world_pick_device(scratch._h, rays_t.numel() // 32, C.c_void_p(rays_t.data_ptr()), C.c_void_p(picks_t.data_ptr()), C.c_void_p(side.cuda_stream)) == 0
    side.synchronize()
    scratch.place_models_device(models, [with_op(i, CARVE) for i in instances], 0)
    return picks_t.cpu().numpy().view(gpu.PICK_HIT_DTYPE)


def with_op(inst, op):
    out = gpu.ModelInstance.from_buffer_copy(bytes(inst))
    out.op = op
    return out


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "model_pick.md")
    ws = host.WorldSet.procedural(dim, dim, dim)
    none = np.zeros(0, dtype=np.int32)
    empty = host.WorldSet.from_voxels(SCRATCH, none, none, none, np.zeros(0, dtype=np.uint32), threads=4)
    ctx, scratch = gpu.Context(0), gpu.Context(0)
    rows, cases = [], []
    try:
        ctx.upload_world(ws)
        scratch.upload_world(empty)
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
        rng = np.random.default_rng(4096)
        side = torch.cuda.Stream()  # (torch's default stream has the handle 0, which cvx_world_pick_device reads as "the context's")
        for bodies in BODIES:
            instances = pile(bodies, [m[0] for m in device_models], rng)
            models = device_models[:min(bodies, len(device_models))]
            for count in RAYS:
                rays = rays_at(instances, count, rng)
                rays_t = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
                hits_t = torch.zeros(count * 48, dtype=torch.uint8, device="cuda")
                picks_t = torch.zeros(count * 24, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                device_ms, wall_ms, hits = timed_calls(ctx, models, instances, rays_t, hits_t, repeats)
                route_ms, same = [], 0.0
                for r in range(min(repeats, 3) + 1):
                    t0 = time.perf_counter()
                    picks = route(scratch, models, instances, rays_t, picks_t, side)
                    if r:
                        route_ms.append((time.perf_counter() - t0) * 1000.0)
                    same = float((picks["voxel"] == hits["voxel"]).all(axis=1).mean())
                row = {"bodies": bodies, "rays": count, "jobs": count_jobs(instances, rays), "hits": int((hits["instance"] >= 0).sum()), "device_ms": device_ms,
                       "wall_ms": wall_ms, "route_ms": stat(route_ms), "route_same": same}
                rows.append(row)
                cases.append((models, instances, rays_t, hits))
                print(json.dumps(row), flush=True)
    finally:
        ctx.close()
        scratch.close()
        ws.close()
        empty.close()
    if os.path.exists(VARIANT):  # the same calls through the lane-per-job build, on a context of its own
        gpu.use_library(VARIANT)
        lanes = gpu.Context(0)
        try:
            for row, (models, instances, rays_t, hits) in zip(rows, cases):
                hits_t = torch.zeros(len(hits) * 48, dtype=torch.uint8, device="cuda")
                row["lane_ms"], _, theirs = timed_calls(lanes, models, instances, rays_t, hits_t, repeats)
                assert theirs.tobytes() == hits.tobytes(), "the lane-per-job build's hits differ from the product's"
                print(json.dumps({"bodies": row["bodies"], "rays": row["rays"], "lane_ms": row["lane_ms"]}), flush=True)
        finally:
            lanes.close()
            gpu.use_library(None)
    lines = ["# cvxq_model_pick: device and wall milliseconds beside the stamp, pick, carve route and a lane-per-job walk (tools/model_pick_bench.py)", "",
             f"{torch.cuda.get_device_name(0)}, bodies lifted from the procedural world {dim}^3 and piled up, medians of {repeats} rounds after a warm-up round "
             f"(min .. max); the route over {min(repeats, 3)} rounds in an empty {SCRATCH[0]}^3 scratch world, LOD 0 only.", "",
             "| bodies | rays | jobs | hits | device ms | wall ms | route ms | route / call (wall) | route names the same voxel | lane-per-job device ms | lane / wave |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        lane = f"{cell(row['lane_ms'])} | {row['lane_ms']['median'] / row['device_ms']['median']:.2f} |" if "lane_ms" in row else "not built | |"
        lines.append(f"| {row['bodies']} | {row['rays']} | {row['jobs']} | {row['hits']} | {cell(row['device_ms'])} | {cell(row['wall_ms'])} | {cell(row['route_ms'])} | "
                     f"{row['route_ms']['median'] / row['wall_ms']['median']:.0f} | {row['route_same']:.3f} | {lane}")
    lines.append("")
    kept = ""
    if os.path.exists(out_path):
        text = open(out_path).read()
        kept = text[text.index(MARKER):] if MARKER in text else ""
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
