"""cvx_world_light on mill512 and on the procedural world of bench.py.
Usage: python tools/light_bench.py [dim] [repeats] ; prints one JSON line per world and case.

Per world, over the whole world and over a 256^3 box around a surface voxel near the middle: the voxels lit, the device_ms of the product (the LDS
brick kernel) and, when cpuvox_amd/libcpuvox_gpu_lightrec.so exists (make -C cpuvox_amd/csrc variant NAME=lightrec DEFS=-DCVX_LIGHT_RECORDS), of the
record-walking variant -- medians of `repeats` calls after one warm-up call, device time from the call's own events, TO_ALPHA so that every repeat
does the same work --, and beside them the route a host had before this call, timed in the same run: cvx_world_read_level of LOD 0 (the host needs
the surroundings of the box too), the sequential driver of tests/light_rules.cpp over the blob (its own milliseconds, without loading the blob),
cvx_world_edit of the rectangle.  Voxels per second for each.  The two libraries' results are compared byte for byte.
sun (3, 5, 2) level 140 range 256, sky level 90 range 6, floor 25.

Then cvx_world_light_lamps on the procedural world: a 256 x dimY x 256 box around the middle with 0, 16, 256 and 4096 lamps of radius 16 scattered
three voxels above the terrain (level 200) and with 16 lamps of radius 64; per lamp set the device time of (a) cvx_world_light on that box, (b) the
new call through the brick kernel, (c) the new call in the record-walking variant, (d) the host route (cvx_world_read_level + the sequential driver
of tests/lamp_rules.cpp + cvx_world_edit), each the median of `repeats` with its min .. max beside it; (voxel, lamp) pairs in range counted on the
host route's blob are not needed for the ratios: the cost per lamp is (b) minus (b) with 0 lamps over the lamp count."""
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
VARIANT = os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu_lightrec.so")
LIGHT = dict(sun_dir=(3, 5, 2), sun_level=140, sun_range=256, sky_level=90, sky_range=6, floor_level=25, target=gpu.LIGHT_TO_ALPHA)
work = tempfile.mkdtemp(prefix="light_bench")
rules, lamp_rules = ruleslib.build("light_rules", work, "-O2"), ruleslib.build("lamp_rules", work, "-O2")


def device(ws, boxes, library):
    """{case: (median device ms, LOD-0 bytes after the calls)} through one library."""
    gpu.use_library(library)
    out = {}
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for case, (lo, hi) in boxes.items():
            ctx.world_light(lo, hi, **LIGHT)  # (warm-up; TO_ALPHA: every later call does the same work on the same world)
            out[case] = (round(float(np.median([ctx.world_light(lo, hi, **LIGHT) for _ in range(repeats)])), 3), ctx.read_level(0)[0])
    finally:
        ctx.close()
        gpu.use_library(None)
    return out


def bench(name, ws):
    dims = tuple(ws.dims)
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    o = np.array([[dims[0] * 0.5 + 0.5, dims[1] - 0.5, dims[2] * 0.5 + 0.5]])
    vox, face, _, _ = ctx.pick(o, np.array([[0.0, -1.0, 0.0]]), float(dims[1]))
    centre = [int(v) for v in vox[0]] if face[0] >= 0 else [dims[0] // 2, dims[1] // 4, dims[2] // 2]
    boxes = {"whole": ([0, 0, 0], list(dims)), "box256": ([max(0, c - 128) for c in centre], [c + 128 for c in centre])}
    product = device(ws, boxes, None)
    variant = device(ws, boxes, VARIANT) if os.path.exists(VARIANT) else None
    for case, (lo, hi) in boxes.items():
        # the route without the call: read LOD 0 back, light it on the host, put the rectangle back
        t = time.perf_counter()
        blob, columns = ctx.read_level(0)
        read_ms = (time.perf_counter() - t) * 1e3
        path, sub = os.path.join(work, "world.bin"), os.path.join(work, "sub.bin")
        open(path, "wb").write(blob)
        words = [*lo, *hi, *LIGHT["sun_dir"], LIGHT["sun_level"], LIGHT["sun_range"], LIGHT["sky_level"], LIGHT["sky_range"], LIGHT["floor_level"], LIGHT["target"], 0]
        text = subprocess.check_output([rules, "world", path, *[str(d) for d in dims], str(columns), *[str(w) for w in words], "5", sub], text=True).split()
        rect = [int(v) for v in text[text.index("rect") + 1:text.index("rect") + 5]]
        voxels, host_ms = int(text[text.index("voxels") + 1]), float(text[text.index("ms") + 1])
        t = time.perf_counter()
        ctx.edit(*rect, open(sub, "rb").read(), rect[2] * rect[3], 5)
        ctx.synchronize()
        edit_ms = (time.perf_counter() - t) * 1e3
        row = {"world": name, "case": case, "voxels": voxels, "lds_device_ms": product[case][0], "lds_mvoxels_per_s": round(voxels / product[case][0] / 1e3, 1)}
        if variant:
            assert variant[case][1] == product[case][1], "the record-walking variant disagrees with the product"
            row.update({"records_device_ms": variant[case][0], "records_mvoxels_per_s": round(voxels / variant[case][0] / 1e3, 1),
                        "records_over_lds": round(variant[case][0] / product[case][0], 2)})
        host_route = read_ms + host_ms + edit_ms
        row.update({"read_level_ms": round(read_ms, 1), "host_light_ms": round(host_ms, 1), "edit_call_ms": round(edit_ms, 1), "host_route_ms": round(host_route, 1),
                    "host_mvoxels_per_s": round(voxels / host_route / 1e3, 2), "host_over_lds": round(host_route / product[case][0], 1), "repeats": repeats})
        assert ctx.read_level(0)[0] == product[case][1], "the host route disagrees with the device"
        print(json.dumps(row), flush=True)
    ctx.close()


def timed(call):
    """(median, min, max) device ms of `repeats` calls after one warm-up."""
    call()
    ms = [call() for _ in range(repeats)]
    return round(float(np.median(ms)), 3), round(min(ms), 3), round(max(ms), 3)


def lamp_bench(name, ws):
    dims = tuple(ws.dims)
    lo, hi = [dims[0] // 2 - 128, 0, dims[2] // 2 - 128], [dims[0] // 2 + 128, dims[1], dims[2] // 2 + 128]
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    rng = np.random.default_rng(7)
    xz = rng.integers(0, 256, size=(4096, 2))
    o = np.stack([lo[0] + xz[:, 0] + 0.5, np.full(4096, dims[1] - 0.5), lo[2] + xz[:, 1] + 0.5], axis=1)
    vox, face, _, _ = ctx.pick(o, np.tile([[0.0, -1.0, 0.0]], (4096, 1)), float(dims[1]))
    ground = [(int(o[k, 0]), (int(vox[k][1]) if face[k] >= 0 else 0) + 3, int(o[k, 2])) for k in range(4096)]
    sets = {f"{n} x r16": [(ground[k], 16, 200) for k in range(n)] for n in (0, 16, 256, 4096)}
    sets["16 x r64"] = [(ground[k], 64, 200) for k in range(16)]
    sun_only = timed(lambda: ctx.world_light(lo, hi, **LIGHT))
    results = {}
    for case, lamps in sets.items():
        results[case] = (timed(lambda: ctx.world_light_lamps(lo, hi, lamps, **LIGHT)), ctx.read_level(0)[0])
    variant = {}
    if os.path.exists(VARIANT):
        gpu.use_library(VARIANT)
        other = gpu.Context(0)
        try:
            other.upload_world(ws)
            for case, lamps in sets.items():
                variant[case] = timed(lambda: other.world_light_lamps(lo, hi, lamps, **LIGHT))
                assert other.read_level(0)[0] == results[case][1], "the record-walking variant disagrees with the product"
        finally:
            other.close()
            gpu.use_library(None)
    for case, lamps in sets.items():
        t = time.perf_counter()
        blob, columns = ctx.read_level(0)
        read_ms = (time.perf_counter() - t) * 1e3
        path, sub, lamp_file = os.path.join(work, "world.bin"), os.path.join(work, "sub.bin"), os.path.join(work, "lamps.bin")
        open(path, "wb").write(blob)
        np.array([[*pos, radius, level] for pos, radius, level in lamps], dtype=np.int32).tofile(lamp_file)
        words = [*lo, *hi, *LIGHT["sun_dir"], LIGHT["sun_level"], LIGHT["sun_range"], LIGHT["sky_level"], LIGHT["sky_range"], LIGHT["floor_level"], LIGHT["target"], 0]
        text = subprocess.check_output([lamp_rules, "world", path, *[str(d) for d in dims], str(columns), *[str(w) for w in words], "5", lamp_file, sub], text=True).split()
        rect = [int(v) for v in text[text.index("rect") + 1:text.index("rect") + 5]]
        voxels, host_ms = int(text[text.index("voxels") + 1]), float(text[text.index("ms") + 1])
        t = time.perf_counter()
        ctx.edit(*rect, open(sub, "rb").read(), rect[2] * rect[3], 5)
        ctx.synchronize()
        edit_ms = (time.perf_counter() - t) * 1e3
        assert ctx.read_level(0)[0] == results[case][1], "the host route disagrees with the device"
        row = {"world": name, "case": "lamps " + case, "voxels": voxels, "sun_only_ms": sun_only, "lamps_lds_ms": results[case][0]}
        if variant:
            row["lamps_records_ms"] = variant[case]
            row["records_over_lds"] = round(variant[case][0] / results[case][0][0], 2)
        row.update({"host_route_ms": round(read_ms + host_ms + edit_ms, 1), "host_light_ms": round(host_ms, 1), "repeats": repeats})
        print(json.dumps(row), flush=True)
    ctx.close()


bench("mill512", scenes.load_world("mill512"))
t0 = time.perf_counter()
ws = host.WorldSet.procedural(dim, dim, dim)
print(json.dumps({"world": f"proc{dim}", "world_build_s": round(time.perf_counter() - t0, 1)}), flush=True)
bench(f"proc{dim}", ws)
lamp_bench(f"proc{dim}", ws)
