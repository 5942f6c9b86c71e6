"""-m gpu: the edge-pose catalogue (tests/edgeposes.py) through the counting build, the batch kernel, the latency kernel and the automatic choice,
every frame against the CPU oracle bit for bit; the catalogue once more in full 64-ray waves of the batch kernel; the entries tagged "repeat"
through the repeat kernels (a repeating world against the same world tiled, tests/test_gpu_world_repeat.py's equivalence).

The oracle renders every frame on the CPU before the frame reaches the GPU (tests/test_edge_poses.py runs it under a time limit)."""
import numpy as np
import pytest

import edgeposes as E
import oraclelib as O
import repeatworld as R
import scenes
import waves
from cpuvox_amd import gpu

pytestmark = pytest.mark.gpu

CLEAR = E.CLEAR
KERNELS = [("batch kernel", gpu.LATENCY_NEVER), ("latency kernel", gpu.LATENCY_ALWAYS), ("automatic choice", gpu.LATENCY_AUTO)]
COUNTERS = ("S", "E", "C", "P", "R")


@pytest.fixture(scope="module")
def contexts():
    cache = {}

    def get(world, W, H):
        if world not in cache:
            ctx = gpu.Context(0)
            ctx.upload_world(E.load_world(world))
            cache[world] = ctx
        ctx = cache[world]
        ctx.set_resolution(W, H)
        return ctx

    yield get
    for ctx in cache.values():
        ctx.close()


def _draw(ctx, fr, mode, counters=False):
    ctx.enable_counters(counters)
    ctx.set_latency_kernel(mode)
    try:
        ctx.clear_raybuffers(0, CLEAR)
        ctx.draw_segments(fr, 0)
    finally:
        ctx.set_latency_kernel(gpu.LATENCY_AUTO)
        ctx.enable_counters(False)
    return ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN), ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)


def _compare(label, fr, g, o):
    n_td, n_lr = scenes.used_rows(fr)
    for part, gb, ob, n in (("topdown", g[0], o[0], n_td), ("leftright", g[1], o[1], n_lr)):
        diff = gb[:n] != ob[:n]
        if diff.any():
            rows, cols = np.nonzero(diff)
            raise AssertionError(f"{label}/{part}: {int(diff.sum())} of {diff.size} pixels differ; first at ray {rows[0]} pixel {cols[0]}: "
                                 f"gpu {gb[rows[0], cols[0]]:08x} oracle {ob[rows[0], cols[0]]:08x}; rays affected {len(set(rows.tolist()))}")
        assert (gb[n:] == CLEAR).all(), f"{label}/{part}: rows beyond the frame's {n} rays were written"


@pytest.mark.parametrize("name", [e.name for e in E.CATALOGUE])
def test_edge_pose_bit_exact(contexts, name):
    e = E.BY_NAME[name]
    ws, fr = E.frame(e)
    o_td, o_lr, cnt, ev = O.draw_segments_events(ws, fr, e.width, e.height, clear=CLEAR)
    for key, least in e.events.items():
        assert getattr(ev, key) >= least, (name, key, ev.as_dict())
    ctx = contexts(e.world, e.width, e.height)
    g = _draw(ctx, fr, gpu.LATENCY_AUTO, counters=True)
    _compare(f"{name} [counting build]", fr, g, (o_td, o_lr))
    gc = ctx.counters()
    assert tuple(getattr(gc, k) for k in COUNTERS) == tuple(getattr(cnt, k) for k in COUNTERS), f"{name} [counting build]: {gc.as_dict()} vs {cnt.as_dict()}"
    assert list(gc.lodVisits) == list(cnt.lodVisits), f"{name} [counting build]"
    for label, mode in KERNELS:
        _compare(f"{name} [{label}]", fr, _draw(ctx, fr, mode), (o_td, o_lr))


def test_edge_poses_in_full_waves(contexts):
    """Every catalogue frame again, in launches of full 64-ray waves (one launch per world and resolution), against the oracle."""
    groups = {}
    for e in E.CATALOGUE:
        groups.setdefault((e.world, e.width, e.height), []).append(e)
    for (world, W, H), entries in groups.items():
        ws = E.load_world(world)
        frames = [E.frame(e)[1] for e in entries]
        oracles = [waves.oracle(ws, fr, W, H) for fr in frames]
        if not any(waves.frame_tile_count(fr) for fr in frames):
            continue
        ctx = contexts(world, W, H)
        waves.check_full_waves(ctx, frames, W, H, f"edge poses {world} {W}x{H}: {', '.join(e.name for e in entries)}", oracles=oracles)


# repeat kernels: world -> (k, far clip).  The camera stands at the entry's position + a tile corner of the k x k tiled world, which keeps integer,
# half-integer and seam positions what they are relative to the tile; the far clip keeps every ray inside the tiled world.
REPEAT_WORLDS = {"proc256": (8, 600.0), "terrace64": (16, 300.0)}


@pytest.mark.parametrize("world", list(REPEAT_WORLDS))
def test_edge_poses_through_repeat_kernels(world):
    entries = [e for e in E.CATALOGUE if "repeat" in e.tags and e.world == world]
    assert entries
    k, far = REPEAT_WORLDS[world]
    ws = E.load_world(world)
    wt = R.tile_world(ws, k)
    c = k * ws.dims[0] // 2
    ctxs = {}
    try:
        for e in entries:
            pos = (c + e.position[0], e.position[1], c + e.position[2])
            assert far + 32 <= min(pos[0], pos[2], k * ws.dims[0] - pos[0], k * ws.dims[2] - pos[2]), e.name
            fr = R.frame(ws, e.width, e.height, pos, e.euler, far, e.lod_error)
            key = (e.width, e.height)
            if key not in ctxs:
                cw, ct = gpu.Context(0), gpu.Context(0)
                cw.upload_world(ws)
                ct.upload_world(wt)
                cw.set_resolution(*key)
                ct.set_resolution(*key)
                cw.set_world_repeat(True)
                ctxs[key] = (cw, ct)
            cw, ct = ctxs[key]
            o_td, o_lr, _ = O.draw_segments(wt, fr, e.width, e.height, clear=CLEAR, counters=False)
            _compare(f"{e.name} tiled x{k} [batch kernel]", fr, _draw(ct, fr, gpu.LATENCY_NEVER), (o_td, o_lr))
            for label, mode in KERNELS:
                _compare(f"{e.name} repeating [{label}]", fr, _draw(cw, fr, mode), (o_td, o_lr))
            got = _draw(cw, fr, gpu.LATENCY_NEVER, counters=True)
            cnt_w = cw.counters().as_dict()
            want = _draw(ct, fr, gpu.LATENCY_NEVER, counters=True)
            cnt_t = ct.counters().as_dict()
            _compare(f"{e.name} repeating [counting build]", fr, got, want)
            assert cnt_w == cnt_t, (e.name, cnt_w, cnt_t)
    finally:
        for pair in ctxs.values():
            for ctx in pair:
                ctx.close()
