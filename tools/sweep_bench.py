"""cvxs_world_sweep_device on the procedural world of bench.py, beside the only route there was before it: cvxc_world_contacts_device for the
poses o_1, o_2, ... of the same path, one blocking call a pose, up to the first pose at which any body overlaps.
Usage: python tools/sweep_bench.py [dim] [repeats] [out.md] ; prints one JSON line per case and writes the table to out.md (default
profiles/sweep.md; the compiler's figures at its head are COMPILER below, taken from the build).

Bodies: tools/contacts_bench.py's -- 32 x 32 loose chunks of 7 x 4 x 7 voxels lifted with cvx_world_lift_pieces_device into torch pools, body k
chunk k mod 256 under a yaw and a tilt of its own -- with their centres `LIFT` voxels above the terrain's surface at places of their own.
Cases: 1, 64 and 1024 bodies, each with the vertical motion (0, -32, 0) and with (12, -32, 7); every body of a case has the same motion.
Before timing, the two routes' answers are compared bit for bit: the first pose the loop stops at is the least `hit` of the sweep, no body
overlaps before it, and the contact results of the bodies that touch there are the sweep's (but for firstPoint, which counts the other bodies'
points).  Rounds interleave the routes: sweep, loop, one contacts call at the start pose, and again.
Columns (milliseconds are medians over `repeats` rounds after a warm-up round, with min .. max):
  sweep device / wall ms   the call's own device time (outDeviceMs, both phases) and the host clock around it
  phase 1 device ms        the same call without contacts: the uploads, the sweep kernel and the read-back of 4 bytes an instance
  contacts device / wall   ONE cvxc_world_contacts_device of the same bodies at the start pose
  loop calls, wall ms      the poses the loop needed and the host clock around all of its calls
  loop / sweep             the two wall medians"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (device arrays; loaded before the library, cpuvox_amd.gpu)
from cpuvox_amd import gpu, host  # noqa: E402
from contacts_bench import CORNER, cell, chunk_strokes, rotation, stat  # noqa: E402

LIFT = 24
CLEAR = 8  # every body can fall this far before it touches: the loop makes more than CLEAR calls
COMPILER = """# cvxs_world_sweep: the compiler's figures and the measured cost (tools/sweep_bench.py)

## The phase 1 kernel as compiled for gfx950

`hipcc -Rpass-analysis=kernel-resource-usage` on cvx_sweep.hip with the Makefile's flags, `cvxsweep::sweep_kernel`:

| VGPRs | AGPRs | SGPRs | SGPR spills (to VGPR lanes) | scratch bytes / lane | LDS bytes | occupancy, waves / SIMD |
|---|---|---|---|---|---|---|
| 42 | 0 | 106 | 44 | 0 | 0 | 7 |

No scratch and no LDS.  The job -- the map's column part, the box, the model's descriptor, the station and the world column's record -- lives on
the scalar side, which is why the scalar file is full and 44 values sit in lanes of spare vector registers; a lane holds its voxel's y, its
candidate and the binary search's bounds.  Phase 2 is cvx_contacts.hip's kernels, unchanged (profiles/contacts.md).

## The early return that was measured and left out

The design allowed a wave to read `first[k]` at its start and return when it is at or below its station's first step.  Three builds of the kernel
on the bodies of the table below, phase 1 alone, device ms (medians of 6 rounds; `rocprofv3 --kernel-trace` on the first build gave the
kernel's own time):

| bodies, motion | agent-scope read (`__hip_atomic_load`) | plain read | no read (shipped) | one contacts call |
|---|---|---|---|---|
| 64, (0, -32, 0) | 0.099 | 0.076 | 0.053 | 0.047 |
| 64, (12, -32, 7) | 0.450 | 0.291 | 0.188 | 0.047 |
| 1024, (0, -32, 0) | 0.651 (kernel 0.56 .. 0.66) | 0.400 | 0.209 | 0.216 (count kernel 0.16 .. 0.17) |
| 1024, (12, -32, 7) | 2.318 (kernel 2.22 .. 2.25) | 2.291 | 2.291 | 0.216 |

The read has to see the other waves' atomics, so it goes past the caches, and every wave waits for it before it can start on its column; on the
motions with a horizontal part it saved nothing, because a wave that returns early has by then done the dependent loads (the prefix search, the
instance, the station) that bound the kernel.  Without the read the vertical sweep's kernel costs what the contacts walk of the same waves costs.
"""
MOTIONS = ((0, -32, 0), (12, -32, 7))


def path_of(motion):
    n = sum(abs(c) for c in motion)
    return [gpu.sweep_offset(motion, j)[0] for j in range(n + 1)]


def loop(ctx, models, poses, results):
    """The parent's route: a contacts call per pose from o_1 on, until a body overlaps -> (the pose's index or -1, the calls made).  poses[j]: the
    instances moved by o_j, made before the clock starts (a host in C moves an instance in a few instructions)."""
    for j in range(1, len(poses)):
        totals, _ = ctx.world_contacts_device(models, poses[j], results)
        if totals["touching"]:
            return j, j
    return -1, len(poses) - 1


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "sweep.md")
    ws = host.WorldSet.procedural(dim, dim, dim)
    ctx = gpu.Context(0)
    rows = []
    try:
        ctx.upload_world(ws)
        y0 = dim - 64
        ctx.brush(chunk_strokes(y0), 5)
        lift_box = ((0, y0 - 1, 0), (CORNER, y0 + 5, CORNER))
        _, totals, _ = ctx.world_lift_pieces_device(*lift_box, gpu.ANCHOR_GROUND, None, None, capacity=0)
        argb = torch.zeros(totals["neededVoxels"], dtype=torch.int32, device="cuda")
        mask = torch.zeros(totals["neededVoxels"], dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pieces, totals, _ = ctx.world_lift_pieces_device(*lift_box, gpu.ANCHOR_GROUND, argb, mask, gpu.LIFT_REMOVE, capacity=1024)
        assert totals["storedPieces"] == 1024 == len(pieces)
        heights, _, _ = ctx.read_heights((0, 0, 0), (dim, dim, dim), want_argb=False)
        model_count = gpu.MODELS_MAX_MODELS
        device_models = [gpu.lifted_model(pieces, k, argb.data_ptr(), mask.data_ptr()) for k in range(model_count)]
        rng = np.random.default_rng(2048)
        for count in (1, 64, 1024):
            instances = []
            for k in range(count):
                size = device_models[k % model_count][0]
                x, z = (int(v) for v in rng.integers(64, dim - 64, size=2))
                linear = rotation(1, float(rng.uniform(0, 360))) @ rotation(0, float(rng.uniform(-20, 20)))
                centre = np.array([x + 0.5, float(heights[x, z]) + LIFT, z + 0.5])
                forward = np.concatenate([linear, (centre - linear @ (np.asarray(size, dtype=np.float64) / 2))[:, None]], axis=1)
                instances.append(gpu.model_instance(forward, size, k % model_count, gpu.BRUSH_FILL))
            models = device_models[:min(count, model_count)]
            contacts = torch.zeros(count * 120, dtype=torch.uint8, device="cuda")
            results = torch.zeros(count * 120, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            for _ in range(8):  # (setup: a body over a slope is raised until it is free CLEAR voxels down and to the side)
                stuck = np.zeros(count, dtype=bool)
                for o in [(0, -d, 0) for d in range(CLEAR + 1)] + [o for o in path_of(MOTIONS[1]) if -o[1] <= CLEAR]:
                    ctx.world_contacts_device(models, [gpu.instance_moved(inst, o) for inst in instances], results)
                    stuck |= results.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE)["overlap"] > 0
                if not stuck.any():
                    break
                for k in np.nonzero(stuck)[0]:
                    instances[k] = gpu.instance_moved(instances[k], (0, 16, 0))
            else:
                raise AssertionError("some bodies could not be freed")
            for motion in MOTIONS:
                poses = [gpu._instance_array([gpu.instance_moved(inst, o) for inst in instances]) for o in path_of(motion)]
                instances = poses[0]
                motions = [motion] * count
                sweep_device, sweep_wall, one_device, one_wall, loop_wall, first_device = [], [], [], [], [], []
                calls = 0
                for r in range(repeats + 1):
                    t0 = time.perf_counter()
                    sweeps, summary, ms = ctx.world_sweep_device(models, instances, motions, contacts)
                    wall = (time.perf_counter() - t0) * 1000.0
                    t0 = time.perf_counter()
                    stopped, calls = loop(ctx, models, poses, results)
                    took = (time.perf_counter() - t0) * 1000.0
                    if r == 0:  # the two routes' answers, bit for bit
                        hits = sweeps["hit"]
                        assert (hits != 0).all(), "no body starts in solid: the loop begins at o_1"
                        assert stopped == (int(hits[hits > 0].min()) if (hits > 0).any() else -1), f"the loop stopped at pose {stopped}, the sweep's least hit is {hits[hits > 0].min()}"
                        if stopped > 0:
                            mine, theirs = contacts.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE).copy(), results.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE).copy()
                            mine["firstPoint"] = theirs["firstPoint"] = 0
                            there = hits == stopped
                            assert there.any() and mine[there].tobytes() == theirs[there].tobytes() and not theirs[~there]["overlap"].any()
                    t0 = time.perf_counter()
                    _, one_ms = ctx.world_contacts_device(models, instances, results)
                    one = (time.perf_counter() - t0) * 1000.0
                    alone, _, first_ms = ctx.world_sweep_device(models, instances, motions)  # phase 1 alone
                    assert alone.tobytes() == sweeps.tobytes()
                    if r:
                        sweep_device.append(ms)
                        sweep_wall.append(wall)
                        loop_wall.append(took)
                        one_device.append(one_ms)
                        first_device.append(first_ms)
                        one_wall.append(one)
                row = {"bodies": count, "motion": list(motion), "jobs": summary["jobs"], "hits": summary["hits"], "first_hit": stopped, "loop_calls": calls,
                       "sweep_device_ms": stat(sweep_device), "phase1_device_ms": stat(first_device), "sweep_wall_ms": stat(sweep_wall), "contacts_device_ms": stat(one_device), "contacts_wall_ms": stat(one_wall),
                       "loop_wall_ms": stat(loop_wall)}
                row["ratio"] = row["loop_wall_ms"]["median"] / row["sweep_wall_ms"]["median"]
                print(json.dumps(row))
                rows.append(row)
    finally:
        ctx.close()
        ws.close()
    lines = [COMPILER, "## Measured", "",
             f"{torch.cuda.get_device_name(0)}, procedural world {dim}^3, bodies {LIFT} voxels above the terrain, medians of {repeats} interleaved rounds after a warm-up "
             f"round (min .. max); every body is free for at least {CLEAR} voxels of its way.  The loop is one cvxc_world_contacts_device a pose from o_1 up to the "
             "first pose at which any body overlaps; its answer was "
             "compared with the sweep's bit for bit before timing.", "",
             "| bodies | motion | jobs | hits | loop calls | sweep device ms | phase 1 alone, device ms | sweep wall ms | one contacts call: device ms | wall ms | loop wall ms | loop / sweep |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        lines.append(f"| {row['bodies']} | {tuple(row['motion'])} | {row['jobs']} | {row['hits']} | {row['loop_calls']} | {cell(row['sweep_device_ms'])} | {cell(row['phase1_device_ms'])} | {cell(row['sweep_wall_ms'])} | "
                     f"{cell(row['contacts_device_ms'])} | {cell(row['contacts_wall_ms'])} | {cell(row['loop_wall_ms'])} | {row['ratio']:.1f} |")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
