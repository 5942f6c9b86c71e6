"""cvx_world_nav_build / cvx_nav_field_goals / cvx_nav_query on the procedural world of bench.py, for a body 1 x 2 x 1 and one 3 x 3 x 3.
Usage: python tools/nav_bench.py [dim] [repeats] [out.md] ; prints one JSON line per width and writes the table to out.md (default
profiles/nav.md).

Per width: cell columns, nodes, reached nodes, largest distance and relax launches of a whole-world build towards two airborne goals (stepUp 1,
maxDrop 3); device_ms and wall-clock ms per call (medians of `repeats`) of the build, of a re-goal (cvx_nav_field_goals with the goals moved)
and of one cvx_nav_query of 65 536 random positions; and, once, the host route the call replaces for the build: cvx_world_read_level of LOD 0
plus the sequential driver of tests/nav_rules.cpp (its own milliseconds, without loading the blob), whose summary is asserted equal."""
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
import ruleslib  # noqa: E402
from cpuvox_amd import gpu, host  # noqa: E402

dim = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "nav.md")
QUERIES = 65536
work = tempfile.mkdtemp(prefix="nav_bench")
rules = ruleslib.build("nav_rules", work, "-O2")


def timed(call):
    t = time.perf_counter()
    result = call()
    return result, (time.perf_counter() - t) * 1e3


def median(values):
    return round(float(np.median(values)), 3)


def bench(ctx, dims, width, height, host_route):
    dx, dy, dz = dims
    whole = ((0, 0, 0), dims)
    goals = [(dx // 2, dy + 1, dz // 2), (dx // 4, dy + 1, dz // 4)]
    moved = [(dx // 2 + 5, dy + 1, dz // 2 - 7), (3 * dx // 4, dy + 1, dz // 4)]
    kw = dict(width=width, height=height, step_up=1, max_drop=3)
    cells = np.random.default_rng(7).integers(0, [dx, dy, dz], size=(QUERIES, 3)).astype(np.int32)
    ctx.nav_build(*whole, goals, **kw).close()  # (warm-up)
    build_ms, build_call, goal_ms, goal_call, query_call = [], [], [], [], []
    for _ in range(repeats):
        field, ms = timed(lambda: ctx.nav_build(*whole, goals, **kw))
        build_ms.append(field.ms)
        build_call.append(ms)
        summary = dict(field.summary)
        _, ms = timed(lambda: field.goals(moved))
        goal_ms.append(field.ms)
        goal_call.append(ms)
        steps, ms = timed(lambda: field.query(cells))
        query_call.append(ms)
        field.close()
    out = {"world": f"proc{dx}", "width": width, "height": height, "cell_columns": (dx - width + 1) * (dz - width + 1), "nodes": summary["nodes"],
           "reached": summary["reached"], "largest_distance": summary["largestDistance"], "relax_launches": summary["launches"],
           "build_device_ms": median(build_ms), "build_call_ms": median(build_call), "regoal_device_ms": median(goal_ms), "regoal_call_ms": median(goal_call),
           "query_65536_call_ms": median(query_call), "resolved_queries": int((steps["cell"][:, 0] >= 0).sum()), "repeats": repeats}
    if host_route:
        (blob, columns), read_ms = timed(lambda: ctx.read_level(0))
        path, goals_path = os.path.join(work, "world.bin"), os.path.join(work, "goals.bin")
        open(path, "wb").write(blob)
        np.asarray(goals, dtype=np.int32).tofile(goals_path)
        text = subprocess.check_output([rules, "world", path, *[str(d) for d in dims], str(columns), "0", "0", "0", *[str(d) for d in dims], str(width), str(height),
                                        "1", "3", "0", goals_path, os.path.join(work, "steps.bin")], text=True).split()
        host_summary = np.frombuffer(open(os.path.join(work, "steps.bin"), "rb").read(40), dtype=gpu.NAV_SUMMARY_DTYPE)[0]
        for name in ("nodes", "reached", "goalsResolved", "largestDistance", "columnsWithSeveralNodes"):
            assert int(host_summary[name]) == summary[name], f"the host route disagrees with the device on {name}"
        out.update({"read_level_ms": round(read_ms, 1), "host_build_ms": float(text[text.index("ms") + 1])})
    print(json.dumps(out), flush=True)
    return out


t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
dims = tuple(ws.dims)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
ctx = gpu.Context(0)
ctx.upload_world(ws)
rows = [bench(ctx, dims, 1, 2, dim <= 512), bench(ctx, dims, 3, 3, False)]
ctx.close()
names = ["width", "height", "cell_columns", "nodes", "reached", "largest_distance", "relax_launches", "build_device_ms", "build_call_ms", "regoal_device_ms",
         "regoal_call_ms", "query_65536_call_ms"]
with open(out_path, "w") as fh:
    fh.write(f"# cvx_world_nav_build, cvx_nav_field_goals, cvx_nav_query: tools/nav_bench.py {dim} {repeats}\n\n")
    fh.write(f"World proc{dim} ({dims[0]} x {dims[1]} x {dims[2]}), whole-world box, two airborne goals, stepUp 1, maxDrop 3; medians of {repeats} runs, milliseconds.\n\n")
    fh.write("| " + " | ".join(names) + " |\n|" + "---|" * len(names) + "\n")
    for row in rows:
        fh.write("| " + " | ".join(str(row[n]) for n in names) + " |\n")
    if "host_build_ms" in rows[0]:
        fh.write(f"\nThe host route for width 1: cvx_world_read_level {rows[0]['read_level_ms']} ms + sequential build {rows[0]['host_build_ms']} ms (same summary).\n")
