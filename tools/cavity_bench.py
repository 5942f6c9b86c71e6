"""cvx_world_cavities on mill512 and on the procedural world of bench.py: the whole world with CVX_CAVITY_OPEN_DEFAULT.
Usage: python tools/cavity_bench.py [dim] [repeats] ; prints one JSON line per world.

Per world: air intervals (nodes), regions and enclosed cavities, device_ms of a REPORT (median of `repeats`) and of a FILL with LOD 1..5 refreshed
(median of `repeats`, each on a fresh upload), and beside them the route a host has without this call, timed in the same run:
cvx_world_read_level of LOD 0 plus the sequential union-find of tests/cavity_rules.cpp over the blob (its own milliseconds, without loading the
blob).  The totals of the two routes are asserted equal.  With the diagnostics build (CVX_GPU_LIB=.../libcpuvox_gpu_exp.so) the analysis / edit
split of the FILL and the hook rounds are added."""
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
import scenes  # noqa: E402
import ruleslib  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OPEN = gpu.CAVITY_OPEN_DEFAULT
ARGB = 0xFF808080
work = tempfile.mkdtemp(prefix="cavity_bench")
rules = ruleslib.build("cavity_rules", work, "-O2")


def bench(name, ws):
    dims = tuple(ws.dims)
    whole = ((0, 0, 0), dims)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    _, summary, _ = ctx.world_cavities(*whole, open_faces=OPEN, capacity=0)  # (warm-up)
    report_ms = round(float(np.median([ctx.world_cavities(*whole, open_faces=OPEN, capacity=64)[2] for _ in range(repeats)])), 3)
    t = time.perf_counter()
    ctx.world_cavities(*whole, open_faces=OPEN, capacity=64)
    report_call_ms = (time.perf_counter() - t) * 1e3
    # the route without the call: read LOD 0 back, union-find on the host
    t = time.perf_counter()
    blob, columns = ctx.read_level(0)
    read_ms = (time.perf_counter() - t) * 1e3
    path = os.path.join(work, "world.bin")
    open(path, "wb").write(blob)
    text = subprocess.check_output([rules, "world", path, *[str(d) for d in dims], str(columns), "0", "0", "0", *[str(d) for d in dims], str(OPEN), "0", str(ARGB), "5",
                                    os.path.join(work, "list.bin"), os.path.join(work, "sub.bin")], text=True).split()
    nodes, host_ms = int(text[text.index("nodes") + 1]), float(text[text.index("ms") + 1])
    host_summary = np.frombuffer(open(os.path.join(work, "list.bin"), "rb").read()[:48], dtype=gpu.CAVITIES_SUMMARY_DTYPE)[0]
    assert {n: int(host_summary[n]) for n in host_summary.dtype.names} == summary, "the host route disagrees with the device"
    fills, calls, split = [], [], {}
    for _ in range(repeats):
        ctx.upload_world(ws)
        t = time.perf_counter()
        _, filled, ms = ctx.world_cavities(*whole, gpu.CAVITIES_FILL, OPEN, 0, ARGB, 5, capacity=0)
        calls.append((time.perf_counter() - t) * 1e3)
        fills.append(ms)
        assert filled == summary
        if hasattr(gpu.lib(), "cvx_debug_cavities"):
            split = ctx.debug_cavities()
    _, after, _ = ctx.world_cavities(*whole, open_faces=OPEN, capacity=0)
    assert after["enclosedCavities"] == 0
    out = {"world": name, "air_intervals": nodes, "regions": summary["enclosedCavities"] + summary["openRegions"], "enclosed": summary["enclosedCavities"],
           "enclosed_voxels": summary["enclosedVoxels"], "report_device_ms": report_ms, "report_call_ms": round(report_call_ms, 3),
           "fill_device_ms": round(float(np.median(fills)), 3), "fill_call_ms": round(float(np.median(calls)), 3),
           "read_level_ms": round(read_ms, 1), "host_union_find_ms": round(host_ms, 1), "host_route_ms": round(read_ms + host_ms, 1), "repeats": repeats}
    if split:
        out.update({"fill_analysis_ms": round(split["analysis_ms"], 3), "fill_edit_ms": round(split["edit_ms"], 3), "hook_rounds": split["rounds"]})
    print(json.dumps(out), flush=True)
    ctx.close()


bench("mill512", scenes.load_world("mill512"))
t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
bench(f"proc{dim}", ws)
