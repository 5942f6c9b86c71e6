"""Repeating worlds (cvx_set_world_repeat) on the GPU.

  python tools/repeat_check.py soak [--poses N] [--seed S]
      random poses: repeat(W) against bounded(T), T = W laid out k x k times with the camera at the same float position inside T (far clip plus
      one LOD-5 cell from its edge), through the latency kernel, the batch kernel and the counting build; prints the mismatching pixels (0 expected).
  python tools/repeat_check.py latency [--world proc2048] [--frames 512] [--reps 20]
      milliseconds per blocking single frame (latency kernel / batch kernel) and per batch of --frames frames at 1080p along the benchmark path,
      repeating with the reference's 10x far clip next to bounded with its 2x.  One JSON line per mode.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import repeatworld as R  # noqa: E402
import scenes  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

W, H = 320, 240


def _draw(ctx, fr, mode):
    ctx.set_latency_kernel(mode)
    ctx.clear_raybuffers(0, 0)
    ctx.draw_segments(fr, 0)
    ctx.set_latency_kernel(gpu.LATENCY_AUTO)
    n_td, n_lr = scenes.used_rows(fr)
    return ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr]


def soak(args):
    rng = np.random.default_rng(args.seed)
    out = {"poses": 0, "pixels": 0, "mismatching_pixels": 0, "mismatching_counters": 0}
    for name, k, far in (("stripes64x64x64", 32, None), ("proc256", 8, 900.0), ("mill256", 8, 900.0)):
        ws = scenes.load_world(name)
        wt = R.tile_world(ws, k)
        D = ws.dims[0]
        c = k * D / 2.0
        room = c - (10.0 * ws.max_dimension if far is None else far) - 33.0
        cw, ct = gpu.Context(0), gpu.Context(0)
        for ctx, world in ((cw, ws), (ct, wt)):
            ctx.upload_world(world)
            ctx.set_resolution(W, H)
        cw.set_world_repeat(True)
        for _ in range(args.poses):
            pos = (c + rng.uniform(-1, 1) * room, rng.uniform(0.05, 1.6) * ws.dims[1], c + rng.uniform(-1, 1) * room)
            eul = (rng.uniform(-60, 89), rng.uniform(0, 360), rng.uniform(-10, 10))
            fr = R.frame(ws, W, H, pos, eul, far, float(rng.choice([1.0, 2.0, 4.0, 8.0])))
            for mode in (gpu.LATENCY_ALWAYS, gpu.LATENCY_NEVER):
                a, b = _draw(cw, fr, mode), _draw(ct, fr, mode)
                out["pixels"] += sum(x.size for x in a)
                out["mismatching_pixels"] += sum(int((x != y).sum()) for x, y in zip(a, b))
            for ctx in (cw, ct):
                ctx.enable_counters(True)
            a, b = _draw(cw, fr, gpu.LATENCY_NEVER), _draw(ct, fr, gpu.LATENCY_NEVER)
            out["mismatching_pixels"] += sum(int((x != y).sum()) for x, y in zip(a, b))
            out["mismatching_counters"] += int(cw.counters().as_dict() != ct.counters().as_dict())
            for ctx in (cw, ct):
                ctx.enable_counters(False)
            out["poses"] += 1
        cw.close()
        ct.close()
    print(json.dumps({"mode": "soak", **out}), flush=True)
    return 0 if out["mismatching_pixels"] == 0 and out["mismatching_counters"] == 0 else 1


def latency(args):
    dim = int(args.world[4:])
    ws = host.WorldSet.procedural(dim, dim, dim, 0x5EED2048)
    Wd, Hd = 1920, 1080
    ctx = gpu.Context(0, buffer_count=args.frames)
    ctx.upload_world(ws)
    ctx.set_resolution(Wd, Hd)
    for repeat in (False, True):
        ctx.set_world_repeat(repeat)
        frames = []
        for i in range(args.frames):
            pos, eul = host.sample_benchmark_path(host.BENCHMARK_PATH_LENGTH * i / args.frames, ws.dims)
            pose = host.camera_pose(pos, eul, Wd, Hd)
            lods, far = host.setup_lods(pose, ws.max_dimension, Wd, Hd, 1.0, repeat=repeat)
            frames.append(host.setup_frame(pose, lods, far, Wd, Hd, ws.dims[1], True))
        row = {"mode": "latency", "world": args.world, "repeat": repeat, "far_clip": frames[0].camera.FarClip}
        for label, kernel in (("single_latency_kernel", gpu.LATENCY_ALWAYS), ("single_batch_kernel", gpu.LATENCY_NEVER)):
            ctx.set_latency_kernel(kernel)
            wall, dev = [], []
            for r in range(args.reps + 2):
                fr = frames[(r * 37) % len(frames)]
                t0 = time.perf_counter()
                ctx.draw_segments(fr, 0)
                t1 = time.perf_counter()
                if r >= 2:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(ctx.last_draw_ms())
            row[label] = {"wall_ms_median": float(np.median(wall)), "kernel_ms_median": float(np.median(dev))}
        ctx.set_latency_kernel(gpu.LATENCY_AUTO)
        times = []
        for r in range(4):
            t0 = time.perf_counter()
            ctx.draw_segments_batch(frames, 0)
            times.append((time.perf_counter() - t0) * 1e3)
        row[f"batch_{args.frames}_ms"] = {"wall_ms_median_of_3": float(np.median(times[1:])), "kernel_ms_last": ctx.last_draw_ms()}
        print(json.dumps(row), flush=True)
    ctx.close()
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("soak", "latency"))
    ap.add_argument("--poses", type=int, default=40, help="soak: poses per world")
    ap.add_argument("--seed", type=int, default=20261015)
    ap.add_argument("--world", default="proc2048")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    return soak(args) if args.mode == "soak" else latency(args)


if __name__ == "__main__":
    sys.exit(main())
