"""cvx_world_move on the procedural world of bench.py.
Usage: python tools/move_bench.py [dim] [repeats] ; prints one JSON line per workload.

Three workloads, every body dropped onto the terrain first and then given one frame's delta (a walk plus gravity, stepUp half a voxel):
  debris   65 536 boxes of 1 x 1 x 1 voxel
  players   4 096 boxes of 0.6 x 1.8 x 0.6 voxel
  boxes       256 boxes of 16 x 4 x 16 voxels
Per workload: the device time of cvx_world_move_device for every lanesPerBody (HIP events around the launch on one stream; min, median and max of
`repeats` launches after a warm-up launch, so that the spread between runs stands beside the figures), the lanesPerBody the host-array call picks
and its wall time (copy in, kernel, copy out), and the route a host had before this call: cvx_world_read_level of LOD 0 once, then the same rule
on the host (tests/move_rules.cpp over the blob, its own milliseconds).  Every route's results are compared byte for byte."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402
import ruleslib  # noqa: E402
from test_world_move_cpu import run_world  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
U = gpu.MOVE_UNIT
LANES = (1, 4, 16, 64)
WORKLOADS = {"debris": (65536, (U, U, U)), "players": (4096, (154, 461, 154)), "boxes": (256, (16 * U, 4 * U, 16 * U))}
work = tempfile.mkdtemp(prefix="move_bench")
rules = ruleslib.build("move_rules", work, "-O2")


def picked(bodies):
    """(largest leg region, lanesPerBody) the host-array call computes for these bodies: asked of the header itself (move_rules lanes)"""
    path = os.path.join(work, "lanes.bin")
    open(path, "wb").write(bodies.tobytes())
    words = subprocess.check_output([rules, "lanes", path], text=True).split()
    return int(words[1]), int(words[3])


t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
ctx = gpu.Context(0)
ctx.upload_world(ws)
t = time.perf_counter()
blob, columns = ctx.read_level(0)
read_ms = (time.perf_counter() - t) * 1e3
stream = torch.cuda.current_stream()
for name, (count, size) in WORKLOADS.items():
    rng = np.random.default_rng(7)
    bodies = np.zeros(count, dtype=gpu.MOVE_BODY_DTYPE)
    bodies["size"] = size
    bodies["pos"][:, 0] = rng.integers(0, (dim - 20) * U, count)
    bodies["pos"][:, 2] = rng.integers(0, (dim - 20) * U, count)
    bodies["pos"][:, 1] = (dim - 8) * U
    bodies["flags"] = gpu.MOVE_SOLID_BELOW | gpu.MOVE_SOLID_SIDES
    for _ in range((dim + 255) // 256):  # the drop: at most 256 voxels per call
        bodies["delta"][:, 1] = -256 * U
        bodies["pos"] = ctx.world_move(bodies)["pos"]
    bodies["delta"][:, 0] = rng.integers(-80, 81, count)
    bodies["delta"][:, 2] = rng.integers(-80, 81, count)
    bodies["delta"][:, 1] = -40
    bodies["stepUp"] = U // 2
    d_bodies = torch.from_numpy(bodies.view(np.int32).reshape(-1, 12).copy()).cuda()
    d_results = torch.zeros((count, 4), dtype=torch.int32, device="cuda")
    ctx.synchronize()
    leg_region, lanes_picked = picked(bodies)
    row = {"workload": name, "bodies": count, "leg_region": leg_region, "repeats": repeats}
    reference = None
    for lanes in LANES:
        times = []
        for k in range(repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctx.world_move_device(count, d_bodies.data_ptr(), d_results.data_ptr(), lanes, stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            if k:
                times.append(a.elapsed_time(b))
        got = d_results.cpu().numpy().tobytes()
        reference = reference or got
        assert got == reference, f"lanesPerBody {lanes} disagrees"
        row[f"g{lanes}_ms"] = [round(float(v), 4) for v in (np.min(times), np.median(times), np.max(times))]
    walls = []
    for k in range(repeats + 1):
        t = time.perf_counter()
        out = ctx.world_move(bodies)
        if k:
            walls.append((time.perf_counter() - t) * 1e3)
    assert out.tobytes() == reference, "the host-array call disagrees"
    want, _, _, host_ms = run_world(rules, __import__("pathlib").Path(work), blob, (dim, dim, dim), columns, False, bodies)
    assert want.tobytes() == reference, "the host rule disagrees with the device"
    row.update({"host_array_lanes": lanes_picked, "host_array_wall_ms": [round(float(v), 3) for v in (np.min(walls), np.median(walls), np.max(walls))],
                "read_level_ms": round(read_ms, 1), "host_rule_ms": round(host_ms, 3),
                "resting": int((want["flags"] & gpu.MOVED_RESTING).astype(bool).sum()), "blocked": int((want["flags"] & 0x33).astype(bool).sum()),
                "stepped": int((want["flags"] & gpu.MOVED_STEPPED).astype(bool).sum())})
    print(json.dumps(row), flush=True)
ctx.close()
