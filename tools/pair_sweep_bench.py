"""cvxm_pair_sweep_device on bodies lifted from the procedural world of bench.py, beside the only route there was before it:
cvxp_model_contacts_device for the poses o_1, o_2, ... of the same path, one blocking call a pose with cvxs_instance_moved on the host in between,
up to the first pose at which any pair overlaps.
Usage: python tools/pair_sweep_bench.py [dim] [repeats] [out.md] ; prints one JSON line per case and writes the table to out.md (default
profiles/pair_sweep.md; the compiler's figures at its head are COMPILER below, taken from the build).

Bodies: tools/pair_contacts_bench.py's -- 32 x 32 loose chunks of 7 x 4 x 7 voxels lifted with cvx_world_lift_pieces_device into torch pools,
body k chunk k mod 256 under a yaw and a tilt of its own -- in a loose pile: that tool's lattice at twice its spacing (12 x 8 x 12 voxels), so
that no two bodies overlap before they move.  The pairs are cvxp_box_pairs' with the largest motion component as the margin (the first 65 536 of
them, the call's limit), the upper body of each as body a; every pair has the same motion of a relative to b.
Cases: 2, 64 and 1024 bodies, each with the motion (0, -32, 0) and with (12, -32, 7).
Before timing, the two routes' answers are compared bit for bit: the first pose the loop stops at is the least `hit` of the sweep, no pair
overlaps before it, and the results of the pairs that touch there are the sweep's contacts (but for a and firstPoint, which name the loop's
moved copy and count the other pairs' points).  Rounds interleave the routes: sweep, loop, one pair-contacts call at the start pose, the sweep
without contacts, and again.
Columns (milliseconds are medians over `repeats` rounds after a warm-up round, with min .. max):
  sweep device / wall ms   the call's own device time (outDeviceMs, both phases) and the host clock around it
  phase 1 device ms        the same call without contacts: the uploads, the sweep kernel and the read-back of 4 bytes a pair
  contacts device / wall   ONE cvxp_model_contacts_device of the same pairs at the start pose
  loop calls, wall ms      the poses the loop needed and the host clock around all of its calls (the moved instances are made before the clock starts)
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

COMPILER = """# cvxm_pair_sweep: the compiler's figures and the measured cost (tools/pair_sweep_bench.py)

## The phase 1 kernel as compiled for gfx950

`hipcc -Rpass-analysis=kernel-resource-usage` on cvx_pair_sweep.hip with the Makefile's flags, `cvxpairsweep::pair_sweep_kernel`:

| VGPRs | AGPRs | SGPRs | SGPR spills (to VGPR lanes) | scratch bytes / lane | LDS bytes | occupancy, waves / SIMD |
|---|---|---|---|---|---|---|
| 66 | 0 | 106 | 93 | 0 | 0 | 7 |

No scratch and no LDS.  Two bodies' column jobs -- each a map's column part in int64, its y column, the box and the model's descriptor --, b's
x and z map columns, the motion, the steps taken and the window of poses live on the scalar side: the scalar file is full and 93 values sit in
lanes of spare vector registers, twice cvx_sweep.hip's 44, which costs vector registers (66 against 42) and no occupancy.  A lane holds its
voxel's y and the three products of the map's finish.  Phase 2 is cvx_pair_contacts.hip's kernels, unchanged (profiles/pair_contacts.md), and a
kernel of a thread a pair that writes the pair's own `a` back into its result.
"""
MOTIONS = ((0, -32, 0), (12, -32, 7))
FILL = gpu.BRUSH_FILL


def loose_pile(count, sizes, rng):
    """tools/pair_contacts_bench.py's pile at twice its spacing: no two bodies overlap."""
    side = int(np.ceil(count ** (1 / 3)))
    instances = []
    for k in range(count):
        size = sizes[k % len(sizes)]
        gx, gz, gy = k % side, (k // side) % side, k // (side * side)
        centre = np.array([16 + 12 * gx, 16 + 8 * gy, 16 + 12 * gz], dtype=np.float64) + rng.uniform(-1, 1, 3)
        linear = rotation(1, float(rng.uniform(0, 360))) @ rotation(0, float(rng.uniform(-20, 20)))
        forward = np.concatenate([linear, (centre - linear @ (np.asarray(size, dtype=np.float64) / 2))[:, None]], axis=1)
        instances.append(gpu.model_instance(forward, size, k % len(sizes), FILL))
    return instances


def path_of(motion):
    n = sum(abs(c) for c in motion)
    return [gpu.sweep_offset(motion, j)[0] for j in range(n + 1)]


def loop(ctx, models, poses, moved_pairs, results):
    """The parent's route: a pair-contacts call per pose from o_1 on, until a pair overlaps -> (the pose's index or -1, the calls made).  poses[j]:
    the instances followed by the same instances moved by o_j; moved_pairs: (count + a, b)."""
    for j in range(1, len(poses)):
        totals, _ = ctx.model_contacts_device(models, poses[j], moved_pairs, results)
        if totals["touching"]:
            return j, j
    return -1, len(poses) - 1


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pair_sweep.md")
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
        model_count = gpu.MODELS_MAX_MODELS
        device_models = [gpu.lifted_model(pieces, k, argb.data_ptr(), mask.data_ptr()) for k in range(model_count)]
        rng = np.random.default_rng(2048)
        for count in (2, 64, 1024):
            bodies = loose_pile(count, [m[0] for m in device_models], rng)
            if count == 2:
                bodies[1] = gpu.instance_moved(bodies[1], (-12, 16, 0))  # the second above the first, not beside it
            models = device_models[:min(count, model_count)]
            for motion in MOTIONS:
                # (b, a) of cvxp_box_pairs' a < b: the pile is built bottom up, so it is the upper body of a pair that moves, down onto the lower
                pairs = np.ascontiguousarray(gpu.box_pairs(bodies, margin=max(abs(c) for c in motion))[:gpu.PAIR_CONTACTS_MAX_PAIRS, ::-1])
                if count == 2:
                    pairs = np.array([[1, 0]], dtype=np.int32)  # the upper one falls
                motions = np.tile(np.asarray(motion, dtype=np.int32), (len(pairs), 1))
                moved_pairs = np.stack([pairs[:, 0] + count, pairs[:, 1]], axis=-1).astype(np.int32)
                poses = [gpu._instance_array(list(bodies) + [gpu.instance_moved(inst, o) for inst in bodies]) for o in path_of(motion)]
                instances = gpu._instance_array(bodies)
                contacts = torch.zeros(len(pairs) * 144, dtype=torch.uint8, device="cuda")
                results = torch.zeros(len(pairs) * 144, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                sweep_device, sweep_wall, one_device, one_wall, loop_wall, first_device = [], [], [], [], [], []
                calls = 0
                for r in range(repeats + 1):
                    t0 = time.perf_counter()
                    sweeps, summary, ms = ctx.model_sweep_device(models, instances, pairs, motions, contacts)
                    wall = (time.perf_counter() - t0) * 1000.0
                    t0 = time.perf_counter()
                    stopped, calls = loop(ctx, models, poses, moved_pairs, results)
                    took = (time.perf_counter() - t0) * 1000.0
                    if r == 0:  # the two routes' answers, bit for bit
                        hits = sweeps["sweep"]["hit"]
                        assert (hits != 0).all(), "no pair starts overlapping: the loop begins at o_1"
                        assert stopped == (int(hits[hits > 0].min()) if (hits > 0).any() else -1), f"the loop stopped at pose {stopped}, the sweep's hits are {sorted(set(hits.tolist()))[:4]}"
                        if stopped > 0:
                            mine, theirs = contacts.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE).copy(), results.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE).copy()
                            mine["firstPoint"] = theirs["firstPoint"] = 0
                            mine["a"] = theirs["a"] = 0
                            there = hits == stopped
                            assert there.any() and mine[there].tobytes() == theirs[there].tobytes() and not theirs[~there]["overlap"].any()
                    t0 = time.perf_counter()
                    _, one_ms = ctx.model_contacts_device(models, instances, pairs, results)
                    one = (time.perf_counter() - t0) * 1000.0
                    alone, _, first_ms = ctx.model_sweep_device(models, instances, pairs, motions)  # phase 1 alone
                    assert alone.tobytes() == sweeps.tobytes()
                    if r:
                        sweep_device.append(ms)
                        sweep_wall.append(wall)
                        loop_wall.append(took)
                        one_device.append(one_ms)
                        first_device.append(first_ms)
                        one_wall.append(one)
                row = {"bodies": count, "pairs": len(pairs), "motion": list(motion), "jobs": summary["jobs"], "hits": summary["hits"], "first_hit": stopped, "loop_calls": calls,
                       "sweep_device_ms": stat(sweep_device), "phase1_device_ms": stat(first_device), "sweep_wall_ms": stat(sweep_wall), "contacts_device_ms": stat(one_device),
                       "contacts_wall_ms": stat(one_wall), "loop_wall_ms": stat(loop_wall)}
                row["ratio"] = row["loop_wall_ms"]["median"] / row["sweep_wall_ms"]["median"]
                print(json.dumps(row), flush=True)
                rows.append(row)
    finally:
        ctx.close()
        ws.close()
    lines = [COMPILER, "## Measured", "",
             f"{torch.cuda.get_device_name(0)}, bodies lifted from the procedural world {dim}^3 in a loose pile, medians of {repeats} interleaved rounds after a warm-up "
             "round (min .. max).  The loop is one cvxp_model_contacts_device a pose from o_1 up to the first pose at which any pair overlaps; its answer was "
             "compared with the sweep's bit for bit before timing.", "",
             "| bodies | pairs | motion | jobs | hits | loop calls | sweep device ms | phase 1 alone, device ms | sweep wall ms | one pair-contacts call: device ms | wall ms | loop wall ms | loop / sweep |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        lines.append(f"| {row['bodies']} | {row['pairs']} | {tuple(row['motion'])} | {row['jobs']} | {row['hits']} | {row['loop_calls']} | {cell(row['sweep_device_ms'])} | "
                     f"{cell(row['phase1_device_ms'])} | {cell(row['sweep_wall_ms'])} | {cell(row['contacts_device_ms'])} | {cell(row['contacts_wall_ms'])} | {cell(row['loop_wall_ms'])} | "
                     f"{row['ratio']:.1f} |")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
