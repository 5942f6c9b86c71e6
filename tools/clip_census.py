"""Diagnostic: which cases of GetWorldBoundsClippingCamSpace the lanes of a wave are in when the frustum clip fails its all-straddle ballot, per
wave execution (needs `make -C cpuvox_amd/csrc gpu-count`; cvxd_clip_census, include/cpuvox_gpu_diag.h).

    python3 tools/clip_census.py [frames = 256]

The benchmark workload (proc2048, 1920 x 1080, benchmark-path poses) in one launch of the batch kernel.  Prints, per pair (class at the Last
intersection, class at the Next one), the executions in which every clipping lane of the wave is in that pair, and, per wave-uniform predicate an
instance of the clip could be keyed on, the executions in which every lane satisfies it / some lanes do / none does."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("CVX_GPU_LIB", os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu_count.so"))
from cpuvox_amd import gpu, host  # noqa: E402

frames_n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
W, H = 1920, 1080
ws = host.WorldSet.procedural(2048, 2048, 2048)
lods, far = host.setup_lods(host.camera_pose((0, 0, 0), (0, 0, 0), W, H), ws.max_dimension, W, H, 1.0)
frames = []
for g in range(frames_n):
    t = ((g * 37) % 1000) / 1000 * host.BENCHMARK_PATH_LENGTH
    pos, eul = host.sample_benchmark_path(t, ws.dims)
    frames.append(host.setup_frame(host.camera_pose(pos, eul, W, H), lods, far, W, H, ws.dims[1]))
ctx = gpu.Context(0, buffer_count=frames_n)
ctx.upload_world(ws)
ctx.set_resolution(W, H)
ctx.debug_section_cycles(reset=True)
ctx.debug_clip_census(reset=True)
ctx.enable_counters(False)
ctx.set_latency_kernel(gpu.LATENCY_NEVER)
ctx.draw_segments_batch(frames, 0)
cyc = ctx.debug_section_cycles()
cen = ctx.debug_clip_census()
ctx.close()

steps, clips, general = cyc[1], cyc[2], cyc[14]
total, arms = cen["executions"], cen["arms"]
print(f"{frames_n} frames, render_kernel<false>: {steps} wave-steps, clip executed {clips} ({clips / max(1, steps):.3f} per wave-step), all-straddle instance "
      f"{cyc[13]} ({cyc[13] / max(1, steps):.3f}), not all-straddle {total} ({total / max(1, steps):.3f}): inverted-straddle instance {arms['inverted_straddle']} "
      f"({arms['inverted_straddle'] / max(1, steps):.3f}), general instance {general} ({general / max(1, steps):.3f}), of those with inverted-straddling lanes "
      f"{arms['general_mixed']} ({arms['general_mixed_lanes'] / max(1, arms['general_mixed']):.1f} such lanes each)")
assert total == arms["inverted_straddle"] + arms["general"] and general == arms["general"] and clips == cyc[13] + total, "the census counts every execution outside the all-straddle instance"
print()
print("The census covers the executions that fail the all-straddle ballot: the general instance as it was before the inverted-straddle instance was split off.")
print("(a) executions in which all clipping lanes share one class pair (Last class, Next class); share of the census executions")
rows = sorted(cen["pairs"].items(), key=lambda kv: -kv[1])
for (cl, cn), n in rows:
    if n:
        print(f"  {gpu.CLIP_CLASSES[cl]:24s} / {gpu.CLIP_CLASSES[cn]:24s} {n:12d}  {n / max(1, total):6.3f}")
uniform = sum(cen["pairs"].values())
print(f"  {'one pair in all lanes':51s} {uniform:12d}  {uniform / max(1, total):6.3f}")
print(f"  {'lanes in different pairs':51s} {cen['mixed_pairs']:12d}  {cen['mixed_pairs'] / max(1, total):6.3f}")
print()
print("(b) wave-uniform predicates (a1 / a2: foot / top above the window's upper bound, b1 / b2: foot / top below its lower bound; at both ends):")
print(f"  {'predicate':78s} {'every lane':>12s} {'share':>6s} {'some lanes':>12s} {'share':>6s} {'lanes/some':>10s}")
for name, text in gpu.CLIP_PREDICATES:
    p = cen["predicates"][name]
    print(f"  {name + ': ' + text:78s} {p['all']:12d} {p['all'] / max(1, total):6.3f} {p['some']:12d} {p['some'] / max(1, total):6.3f} {p['some_lanes'] / max(1, p['some']):10.1f}")
