"""cvxp_model_contacts_device on bodies lifted from the procedural world of bench.py, beside the only route a host has without the call: per pair
(a, b) FILL b into an empty scratch world with cvx_world_place_models_device, ask cvxc_world_contacts_device for a, and CARVE b out again.
Usage: python tools/pair_contacts_bench.py [dim] [repeats] [out.md] ; prints one JSON line per case and writes the table to out.md (default
profiles/pair_contacts.md; whatever follows a line "## Kernel resources" in an existing file is kept).

Bodies: tools/contacts_bench.py's 1024 loose chunks of 7 x 4 x 7 voxels, lifted with cvx_world_lift_pieces_device (REMOVE) into torch pools: body k
is chunk k mod 256 (a call takes 256 models) under a yaw and a tilt of its own, in a pile: a lattice 6 x 3 x 6 voxels apart with a jitter of a
voxel, so that neighbours interpenetrate.  The pairs are those cvxp_box_pairs finds (its own host time is in the table); one body has no pair,
so the smallest case is 2 bodies.
Cases: 2, 64 and 1024 bodies, results alone (pointCapacity 0) and with every contact point.
Columns (milliseconds are medians over `repeats` rounds after a warm-up round, with min .. max):
  device ms   the call's own device time (outDeviceMs)
  wall ms     the host clock around the call, which returns when the summary is on the host
  route ms    the stamp, contacts, carve route on the first `route pairs` pairs (as many as stay within a few seconds), host clock around the
              loop, each call of which returns when its work is done; its overlaps are compared with the call's in the warm-up round
  per pair    route ms / route pairs beside wall ms / pairs, and their ratio"""
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

FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE
SCRATCH = (128, 128, 128)  # the empty world of the route: the pile of 1024 bodies is 11 x 11 x 9 bodies 6 x 3 x 6 voxels apart
ROUTE_PAIRS = 4096
MARKER = "## Kernel resources"


def pile(count, sizes, rng):
    """Instances of `count` bodies in a pile inside SCRATCH, op FILL."""
    side = int(np.ceil(count ** (1 / 3)))
    instances = []
    for k in range(count):
        size = sizes[k % len(sizes)]
        gx, gz, gy = k % side, (k // side) % side, k // (side * side)
        centre = np.array([16 + 6 * gx, 16 + 3 * gy, 16 + 6 * gz], dtype=np.float64) + rng.uniform(-1, 1, 3)
        linear = rotation(1, float(rng.uniform(0, 360))) @ rotation(0, float(rng.uniform(-20, 20)))
        forward = np.concatenate([linear, (centre - linear @ (np.asarray(size, dtype=np.float64) / 2))[:, None]], axis=1)
        instances.append(gpu.model_instance(forward, size, k % len(sizes), FILL))
    return instances


def with_op(inst, op):
    out = gpu.ModelInstance.from_buffer_copy(bytes(inst))
    out.model, out.op = 0, op
    return out


def route(scratch, models, instances, pairs, result):
    """Stamp b, ask for a, carve b: one edit pipeline and one contacts call per pair -> the overlaps."""
    overlaps = []
    for a, b in pairs:
        model_a, model_b = [models[instances[a].model]], [models[instances[b].model]]
        scratch.place_models_device(model_b, [with_op(instances[b], FILL)], 0)
        totals, _ = scratch.world_contacts_device(model_a, [with_op(instances[a], FILL)], result, None, 0)
        scratch.place_models_device(model_b, [with_op(instances[b], CARVE)], 0)
        overlaps.append(totals["overlap"])
    return overlaps


def main():
    dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "pair_contacts.md")
    ws = host.WorldSet.procedural(dim, dim, dim)
    none = np.zeros(0, dtype=np.int32)
    empty = host.WorldSet.from_voxels(SCRATCH, none, none, none, np.zeros(0, dtype=np.uint32), threads=4)
    ctx, scratch = gpu.Context(0), gpu.Context(0)
    rows = []
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
        model_count = gpu.MODELS_MAX_MODELS
        device_models = [gpu.lifted_model(pieces, k, argb.data_ptr(), mask.data_ptr()) for k in range(model_count)]
        rng = np.random.default_rng(2048)
        one_result = torch.zeros(120, dtype=torch.uint8, device="cuda")
        for count in (2, 64, 1024):
            instances = pile(count, [m[0] for m in device_models], rng)
            models = device_models[:min(count, model_count)]
            t0 = time.perf_counter()
            pairs = gpu.box_pairs(instances)
            broad_ms = (time.perf_counter() - t0) * 1000.0
            pairs = pairs[:gpu.PAIR_CONTACTS_MAX_PAIRS]
            results = torch.zeros(len(pairs) * 144, dtype=torch.uint8, device="cuda")
            totals, _ = ctx.model_contacts_device(models, instances, pairs, results)
            points = torch.zeros(max(totals["points"], 1) * 32, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert totals["touching"] >= 1, totals
            route_pairs = pairs[:ROUTE_PAIRS]
            for with_points in (False, True):
                device_ms, wall_ms, route_ms = [], [], []
                for r in range(repeats + 1):
                    t0 = time.perf_counter()
                    got, ms = ctx.model_contacts_device(models, instances, pairs, results, points if with_points else None)
                    wall = (time.perf_counter() - t0) * 1000.0
                    assert got == totals
                    if r <= min(repeats, 3) and not with_points:
                        t0 = time.perf_counter()
                        overlaps = route(scratch, models, instances, route_pairs, one_result)
                        took = (time.perf_counter() - t0) * 1000.0
                        if r == 0:
                            mine = results.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE)["overlap"][:len(route_pairs)]
                            assert overlaps == mine.tolist(), "the route's overlaps differ from the call's"
                        else:
                            route_ms.append(took)
                    if r:
                        device_ms.append(ms)
                        wall_ms.append(wall)
                row = {"bodies": count, "pairs": len(pairs), "touching": totals["touching"], "jobs": totals["jobs"], "points": with_points, "overlap": totals["overlap"],
                       "listed": totals["points"] if with_points else 0, "box_pairs_ms": broad_ms, "device_ms": stat(device_ms), "wall_ms": stat(wall_ms)}
                if route_ms:
                    row["route_pairs"], row["route_ms"] = len(route_pairs), stat(route_ms)
                    row["route_per_pair_ms"] = row["route_ms"]["median"] / len(route_pairs)
                    row["per_pair_ms"] = row["wall_ms"]["median"] / len(pairs)
                    row["ratio"] = row["route_per_pair_ms"] / row["per_pair_ms"]
                print(json.dumps(row))
                rows.append(row)
    finally:
        ctx.close()
        scratch.close()
        ws.close()
        empty.close()
    lines = ["# cvxp_model_contacts: device and wall milliseconds beside the stamp, contacts, carve route (tools/pair_contacts_bench.py)", "",
             f"{torch.cuda.get_device_name(0)}, bodies lifted from the procedural world {dim}^3 and piled up, medians of {repeats} rounds after a warm-up round "
             f"(min .. max); the route over {min(repeats, 3)} rounds on the first pairs of the same list, in an empty {SCRATCH[0]}^3 scratch world, LOD 0 only.", "",
             "| bodies | pairs (touching) | jobs | points listed | overlap | box_pairs ms | device ms | wall ms | route pairs | route ms | route / call, per pair |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        tail = (f"{row['route_pairs']} | {cell(row['route_ms'])} | {row['route_per_pair_ms']:.3f} / {row['per_pair_ms']:.5f} ms = {row['ratio']:.0f} |" if "route_ms" in row
                else "| | |")
        lines.append(f"| {row['bodies']} | {row['pairs']} ({row['touching']}) | {row['jobs']} | {row['listed'] if row['points'] else 'none (capacity 0)'} | {row['overlap']} | "
                     f"{row['box_pairs_ms']:.3f} | {cell(row['device_ms'])} | {cell(row['wall_ms'])} | {tail}")
    lines += ["", "The route is timed on the results-alone rows only (it lists no points of its own in this comparison); each of its pairs is two edit pipelines and one "
              "contacts call, every one of which waits for the device, so its cost is the host's round trips far more than device work.", ""]
    kept = ""
    if os.path.exists(out_path):
        text = open(out_path).read()
        kept = text[text.index(MARKER):] if MARKER in text else ""
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n" + kept)


if __name__ == "__main__":
    main()
