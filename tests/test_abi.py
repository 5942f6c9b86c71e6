"""CPU: what the built libraries, the reference's struct layouts and bench.py's plumbing must hold without a GPU (no compute here).  That the
libraries export what their headers declare is tests/test_abi_mirrors.py's."""
import os

import pytest

import abilib
from cpuvox_amd import gpu, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_product_abi_has_no_diagnostic_entry_points():
    """The drop-in boundary is include/cpuvox_gpu.h; section profiles, the occupancy query and the arithmetic self-test live in
    include/cpuvox_gpu_diag.h and in the experiment / profiling builds only.  Which library exports which header's list is
    tests/test_abi_mirrors.py's to say; here: neither the header's text nor the product library's bytes speak of them."""
    header = open(os.path.join(ROOT, "include", "cpuvox_gpu.h")).read()
    assert "debug" not in header.lower() and "selftest" not in header.lower()
    data = open(os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu.so"), "rb").read()
    assert b"cvx_debug" not in data and b"selftest" not in data


def test_struct_layouts_match_the_reference_blittable_layout():
    """The sizes and offsets of the original's own structs, which no header states: pinned for the header's field list (laid out by
    tests/abilib.py) and for the ctypes classes alike."""
    _, structs, _ = abilib.abi()
    # RenderManager.SegmentData (RenderManager.cs:503-510): 4 float2 + int = 36 bytes
    slots, total, _ = abilib.layout(structs["cvx_segment_data"].fields, structs)
    assert (slots, total) == abilib.ctypes_layout(host.SegmentData) and total == 36
    # CameraData (CameraData.cs:11-16): float4x4 + float2 + float + bool(+3) + float + float[6] = 108 bytes
    slots, total, _ = abilib.layout(structs["cvx_camera_data"].fields, structs)
    assert (slots, total) == abilib.ctypes_layout(host.CameraData) and total == 108
    offsets = {s.name: s.offset for s in slots}
    assert offsets["InverseElementIterationDirection"] == 76
    assert offsets["FarClip"] == 80 and offsets["LODDistances"] == 84


def test_gpu_code_object_is_gfx950():
    data = open(gpu.lib_path(), "rb").read()
    assert b"gfx950" in data


def test_product_library_reads_no_environment_and_holds_one_render_kernel():
    """`strings libcpuvox_gpu.so | grep CVX_` is empty: no diagnostic environment switch, no experiment kernel in the shipped library
    (those live in the -DCVX_EXPERIMENTS build, libcpuvox_gpu_exp.so, which the tests of the switches load explicitly)."""
    data = open(os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu.so"), "rb").read()
    assert b"CVX_" not in data
    assert b"getenv" not in data, "the product library must not look at the caller's environment"
    assert b"render_sm_kernel" not in data
    assert data.count(b"_ZN4cvxk13render_kernelILb0E") > 0 and data.count(b"_ZN4cvxk13render_kernelILb1E") > 0
    exp = os.path.join(ROOT, "cpuvox_amd", "libcpuvox_gpu_exp.so")
    if os.path.exists(exp):
        assert b"CVX_TILE_SPLIT" in open(exp, "rb").read()


def test_product_fails_loudly_without_a_device():
    """No CPU fallback: without a HIP device context creation raises (on a GPU box it succeeds)."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(gpu.CvxError):
        gpu.Context(0)


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "cpuvox_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp", "Makefile")):
                text = open(os.path.join(root, f), errors="ignore").read()
                assert "oraclelib" not in text and "cvx_oracle" not in text and "libcvx_oracle" not in text, os.path.join(root, f)


@pytest.mark.parametrize("world_size", [1, 2, 3, 8])
def test_native_shard_plan_matches_the_python_plan(world_size):
    """cvx_shard_plan_* (the multi-GPU plan behind the C ABI, no GPU needed) against cpuvox_amd.dist.ShardPlan: same tile
    count, same section boundaries, same output address for every tile, for every rank."""
    import ctypes as C

    import numpy as np

    import scenes
    from cpuvox_amd import dist as cdist

    W, H = 640, 480
    ws = scenes.load_world("proc256")
    frames = [scenes.benchmark_frame(ws, W, H, t, 4.0) for t in (0.0, 0.2, 0.45, 0.6, 0.75, 0.8, 0.9, 1.0, 1.1, 0.33, 0.66)]
    n = len(frames)
    segs = (host.SegmentData * (4 * n))()
    cams = (host.CameraData * n)()
    vps = (C.c_float * (2 * n))()
    for i, f in enumerate(frames):
        for s in range(4):
            segs[4 * i + s] = f.segments[s]
        cams[i] = f.camera
        vps[2 * i], vps[2 * i + 1] = f.vanishingPointScreenSpace[0], f.vanishingPointScreenSpace[1]
    packed = (n, segs, cams, vps)
    send_base, disp_base = 0x7F0000000000, 0x7E0000000000
    rendered = np.zeros(0, dtype=np.int64)
    for rank in range(world_size):
        ref = cdist.ShardPlan(frames, W, H, rank, world_size)
        nat = gpu.NativeShardPlan(packed, W, H, rank, world_size)
        assert nat.tile_count == ref.tile_count
        assert np.array_equal(nat.send_start, ref.send_start) and np.array_equal(nat.disp_start, ref.disp_start)
        a, b = nat.tile_out(send_base, disp_base), ref.tile_out(send_base, disp_base)
        assert np.array_equal(a, b)
        rendered = np.concatenate([rendered, np.flatnonzero(a)])
        # what cvx_exchange sends / receives per peer == the slices the Python exchange hands to isend / irecv, and the two sides of
        # every pair agree on the size (rank r sends to p exactly what p expects from r)
        for peer in range(world_size):
            s0, sn, r0, rn = nat.transfer(peer)
            if peer == rank:
                assert (sn, rn) == (0, 0)
                continue
            assert (s0, sn) == (int(ref.send_start[peer]), int(ref.send_start[peer + 1] - ref.send_start[peer]))
            assert (r0, rn) == (int(ref.disp_start[peer]), int(ref.disp_start[peer + 1] - ref.disp_start[peer]))
            other = cdist.ShardPlan(frames, W, H, peer, world_size)
            assert sn == int(other.disp_start[rank + 1] - other.disp_start[rank]) and rn == int(other.send_start[rank + 1] - other.send_start[rank])
        nat.close()
    # every tile of the batch is rendered by exactly one rank
    assert np.array_equal(np.sort(rendered), np.arange(ref.tile_count))


def test_exchange_entry_points_fail_cleanly_without_a_device_or_peers():
    """cvx_exchange / cvx_comm_*: argument errors are reported, nothing is dereferenced (the data path needs >= 2 GPUs)."""
    L = gpu.lib()
    assert L.cvx_exchange(None, None, None, None, None, None) == -1      # CVX_ERR_INVALID_ARGUMENT: no context
    assert L.cvx_comm_create(None, None, 0, 1, None) == -1
    assert L.cvx_comm_unique_id(None) == -1
    assert L.cvx_comm_destroy(None) == 0
    assert L.cvx_shard_plan_tile_count(None) == 0


def test_bench_attaches_the_committed_counter_summary_of_this_library():
    """bench.py's `roofline.traffic` comes from profiles/rNN_pmc_render_kernel*.csv, matched by the sha-256 of the library it loads and by the workload
    arguments.  When the tree's library is the one the newest profiles were collected with, the default workload must find its file
    (round 4: the lookup referenced a name that did not exist at module level and silently returned None)."""
    import argparse
    import importlib.util
    import json

    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    sys_path = os.path.join(ROOT, "tools")
    import sys
    sys.path.insert(0, sys_path)
    from pmc_aggregate import library_sha256

    newest = sorted(p for p in os.listdir(os.path.join(ROOT, "profiles")) if p.endswith("_pmc_render_kernel.csv"))[-1]
    stamp = json.loads(open(os.path.join(ROOT, "profiles", newest)).readline()[1:])
    args = argparse.Namespace(frames=512, width=1920, height=1080, world="proc2048", lod_error=1.0, pose_range=None, steps=10, warmup=2)
    found = bench.find_counter_summary(args)
    if stamp.get("library_sha256") == library_sha256(gpu.lib_path()):
        assert found and os.path.basename(found) == newest, found
    else:
        assert found is None or os.path.basename(found) != newest  # another build: its counters are not this library's


def test_counter_summary_serves_the_drivers_argument_vector(tmp_path, monkeypatch):
    """the driver runs `bench.py --gpus 1 --steps 20 --warmup 5`, the builder's default is 10 / 2 -- and round 4's summary,
    collected with the default, was refused for the driver's line (`roofline.traffic: null`).  A summary now lists every launch, bench.py takes
    the mean over the timed steps of ITS run; both argument vectors must find the file, a longer run than the collected one must not."""
    import importlib.util
    import json
    import sys

    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from pmc_aggregate import library_sha256

    (tmp_path / "profiles").mkdir()
    stamp = {"kernel_sources_sha256": "x", "library_sha256": library_sha256(gpu.lib_path()),
             "bench_args": ["--cpu-seconds", "0", "--latency-frames", "0", "--steps", "20", "--warmup", "5"]}
    fetch = [1000.0 + i for i in range(25)]
    write = [10.0 * (i % 2) for i in range(25)]
    with open(tmp_path / "profiles" / "r99_pmc_render_kernel.csv", "w") as fh:
        fh.write("# " + json.dumps(stamp) + "\n")
        fh.write("counter,mean_per_launch,launches,per_launch\n")
        fh.write("FETCH_SIZE,%g,25,%s\n" % (sum(fetch) / 25, ";".join("%.9g" % v for v in fetch)))
        fh.write("WRITE_SIZE,%g,25,%s\n" % (sum(write) / 25, ";".join("%.9g" % v for v in write)))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.delenv("CVX_GPU_LIB", raising=False)

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])  # the driver's command line, verbatim
    args = bench.parse_args()
    found = bench.find_counter_summary(args)
    assert found and found.endswith("r99_pmc_render_kernel.csv"), found
    c = bench.read_counter_summary(found, args.warmup, args.steps)
    assert c["FETCH_SIZE"] == sum(fetch[5:25]) / 20 and c["WRITE_SIZE"] == sum(write[5:25]) / 20

    monkeypatch.setattr(sys, "argv", ["bench.py"])  # the default run: steps 2 .. 11 of the same launches
    args = bench.parse_args()
    found = bench.find_counter_summary(args)
    assert found, "the default --steps 10 --warmup 2 is covered by the 25 collected launches"
    assert bench.read_counter_summary(found, args.warmup, args.steps)["FETCH_SIZE"] == sum(fetch[2:12]) / 10

    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "30", "--warmup", "5"])  # longer than what was collected: no counters for steps 25 ..
    assert bench.find_counter_summary(bench.parse_args()) is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "20", "--warmup", "5", "--width", "3840", "--height", "2160"])  # another workload
    assert bench.find_counter_summary(bench.parse_args()) is None
    # a summary of rounds 1-4 (no per-launch column) still serves exactly the run that collected it, nothing else
    old = os.path.join(ROOT, "profiles", "r04_pmc_render_kernel.csv")
    assert bench.read_counter_summary(old, 2, 10) is not None and bench.read_counter_summary(old, 5, 20) is None


def test_bench_dump_outputs_hold_the_written_pixels_only(tmp_path, monkeypatch):
    """bench.py --dump-outputs: a fixed sample of the pixels the last step's frames WRITE (never a raybuffer's stale rest), as float arrays of at
    most 64 MB, the same bytes for the same raybuffers.  The raybuffers here are the CPU oracle's, pre-cleared to a marker colour where a frame
    writes nothing, served through a stand-in for the device context."""
    import importlib.util
    import sys

    import numpy as np
    import oraclelib as O
    import scenes
    from cpuvox_amd import dist as cdist

    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "a")])
    args = bench.parse_args()
    assert (args.steps, args.warmup, args.dump_outputs) == (3, 1, str(tmp_path / "a"))
    for bad in (["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", str(tmp_path / "x")]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + bad)
        with pytest.raises(SystemExit):
            bench.parse_args()

    marker = 0xDEADBEEF
    ws, fr, W, H = scenes.scene_frame("proc256_t075_lod8")
    td, lr, _ = O.draw_segments(ws, fr, W, H, clear=marker)

    class Ctx:
        def read_raybuffer(self, b, which, first, n):
            return (td if which == gpu.RAYBUFFER_TOPDOWN else lr)[first:first + n].copy()

    frames = [fr] * 20
    for d in ("a", "b"):
        bench.dump_outputs(Ctx(), frames, W, H, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["frame_index.npy", "raybuffer_channel_sums.npy", "raybuffer_sample.npy", "written_pixels.npy"]
    out = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    for n in names:
        assert np.array_equal(out[n[:-4]], np.load(tmp_path / "b" / n)), n

    assert list(out["frame_index"]) == [0, 2, 5, 7, 10, 12, 15, 17]
    sample = out["raybuffer_sample"]
    assert sample.shape == (8, bench.DUMP_SAMPLE) and (sample >= 0).all() and not (sample == marker).any()
    rc = [max(0, sg.RayCount) for sg in fr.segments]
    row0 = [0, rc[0], 0, rc[2]]
    for sg, (lo, hi) in enumerate(cdist.segment_pixel_ranges(fr.vanishingPointScreenSpace, W, H)):
        part = (td if sg < 2 else lr)[row0[sg]: row0[sg] + rc[sg], lo: hi + 1]
        assert (out["written_pixels"][:, sg] == part.size).all()
        assert (out["raybuffer_channel_sums"][:, sg] == part.reshape(-1, 1).view(np.uint8).sum(axis=0)).all()
    assert set(np.unique(sample[0])) <= set(np.unique(np.concatenate([td.ravel(), lr.ravel()])).tolist()) - {marker}


def test_bench_full_is_off_by_default_and_owns_the_counter_summary(monkeypatch):
    """A plain bench.py run does only what its headline needs; --full (off by default) adds the instrumented pass, the roofline and the legs beside
    it.  --pmc-csv only fills the roofline of a --full run, so on its own it is an argument error rather than a flag that is silently dropped."""
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--pmc-csv", "x.csv"])
    args = bench.parse_args()
    assert args.full is True and args.pmc_csv == "x.csv"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--pmc-csv", "x.csv"])
    with pytest.raises(SystemExit):
        bench.parse_args()


def test_gpu_objects_do_not_depend_on_the_build_directory(tmp_path):
    """bench.py attaches the committed counter summary only to the library whose sha-256 it is stamped with, and the GPU box rebuilds stale targets at
    its own scratch path: the product library's objects are compiled with a fixed compilation-unit id (csrc/Makefile), so the same sources give the
    same bytes in any directory.  Checked on the smallest translation unit, built through the Makefile's own rule in two places."""
    import hashlib
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc here")
    digests = []
    for name in ("a", "somewhere/else"):
        tree = tmp_path / name
        shutil.copytree(os.path.join(root, "cpuvox_amd", "csrc"), tree / "cpuvox_amd" / "csrc", ignore=shutil.ignore_patterns(".obj", "*.o", "*.so"))
        shutil.copytree(os.path.join(root, "include"), tree / "include")
        obj = tree / "cpuvox_amd" / "csrc" / ".obj" / "product" / "cvx_shard.o"
        subprocess.run(["make", "-C", str(tree / "cpuvox_amd" / "csrc"), str(obj)], check=True, capture_output=True, text=True, timeout=600)
        digests.append(hashlib.sha256(obj.read_bytes()).hexdigest())
    assert digests[0] == digests[1]
