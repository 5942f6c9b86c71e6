"""-m gpu: which kernel instance and which wave shape a draw gets (cvx_gpu.hip DrawBatch), read back through cvx_debug_last_launch of the
experiment build.  The parity tests rely on these shapes -- the full-wave passes (tests/waves.py) on 64 different rays per wave, the pinned
kernels on their instance, the forced splits on their dupShift -- so a budget that moves makes THIS test fail instead of quietly hollowing
out the others.  Thresholds come from the frames' tile / ray counts and the device's CU count, never from frame counts."""
import os

import pytest

import scenes
import waves
from cpuvox_amd import gpu

pytestmark = pytest.mark.gpu

W, H = 320, 200
LONE_RAYS = 12288  # AUTO: launches of at most this many rays (tiles x 64) go to the latency kernel; three quarters of it above 2560 x 1440


@pytest.fixture
def exp_ctx():
    path = os.path.join(os.path.dirname(gpu.lib_path()), "libcpuvox_gpu_exp.so")
    assert os.path.exists(path), "libcpuvox_gpu_exp.so not built: run `make -C cpuvox_amd/csrc all` (or __graft_entry__.build())"
    gpu.use_library(path)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(scenes.load_world("proc256"))
        yield ctx
    finally:
        ctx.close()
        gpu.use_library(None)


def _path_frames(width, height):
    ws = scenes.load_world("proc256")
    return [scenes.benchmark_frame(ws, width, height, t, 6.0) for t in (0.0, 0.3, 0.45, 0.55, 0.75, 0.9, 1.1)]


def _level_frames(width, height):
    """Cameras looking level (forward.y clamped to +-0.001): one segment each, few tiles."""
    ws = scenes.load_world("proc256")
    return [scenes.make_frame(ws, width, height, (40.3 + 30 * i, 150.0, 60.2 + 20 * i), (0.0, 20.0 + 50 * i, 0.0)) for i in range(4)]


def _launch(ctx, frames, width, height, latency, counters=False):
    if ctx.width != width or ctx.height != height:
        ctx.set_resolution(width, height)
    if ctx.buffer_count < len(frames):
        ctx.set_buffer_count(len(frames))
    ctx.enable_counters(counters)
    ctx.set_latency_kernel(latency)
    try:
        ctx.draw_segments_batch(frames, 0)
    finally:
        ctx.set_latency_kernel(gpu.LATENCY_AUTO)
        ctx.enable_counters(False)
    shape = ctx.debug_last_launch()
    tiles = sum(waves.frame_tile_count(f) for f in frames)
    assert shape["tiles"] == tiles, (shape, tiles)
    return shape


def test_counters_select_the_counting_instance_in_every_mode(exp_ctx):
    frames = _path_frames(W, H)[:1]
    for mode in (gpu.LATENCY_AUTO, gpu.LATENCY_NEVER, gpu.LATENCY_ALWAYS):
        shape = _launch(exp_ctx, frames, W, H, mode, counters=True)
        assert shape["instance"] == gpu.INSTANCE_COUNTING, (mode, shape)
        assert shape["max_dup_shift"] == 0, shape  # (the counting build sums over lanes: it never duplicates them)


def test_never_selects_the_batch_kernel(exp_ctx):
    for fr in _path_frames(W, H):
        shape = _launch(exp_ctx, [fr], W, H, gpu.LATENCY_NEVER)
        assert shape["instance"] == gpu.INSTANCE_BATCH, shape
        # ... and a lone frame is exactly what the full-wave passes exist for: one or two rays per wave, copied into all 64 lanes
        split = waves.expected_split(shape["tiles"])
        assert split >= 32 and shape["split"] == split and shape["max_rays"] == 64 // split and 1 << shape["max_dup_shift"] == split, shape


@pytest.mark.parametrize("width,height", [(320, 200), (640, 480)])
def test_full_wave_batch_gives_64_rays_to_every_wave(exp_ctx, width, height):
    frames = _path_frames(width, height)
    assert max(max(waves.frame_mask_words(f, width, height)) for f in frames) * 64 <= 40 * 64, "every tile must fit the smallest LDS budget"
    batch, buffers = waves.full_wave_batch(frames)
    assert buffers == len(batch)
    budget = waves.wave_budget()
    for mode in (gpu.LATENCY_NEVER, gpu.LATENCY_AUTO):
        shape = _launch(exp_ctx, batch, width, height, mode)
        msg = f"{width}x{height} {len(batch)} frames, CU budget {budget} waves: launch {shape}"
        assert shape["tiles"] * 2 > budget, msg
        assert shape["instance"] == gpu.INSTANCE_BATCH, msg
        assert shape["split"] == 1 and shape["min_rays"] == 64 and shape["max_rays"] == 64 and shape["max_dup_shift"] == 0, msg
        assert shape["waves"] == shape["tiles"], msg


@pytest.mark.parametrize("split", [2, 4, 16, 64])
def test_split_batch_lands_on_its_split(exp_ctx, split):
    batch, _ = waves.split_batch(_path_frames(W, H), split)
    shape = _launch(exp_ctx, batch, W, H, gpu.LATENCY_NEVER)
    msg = f"split {split}, {len(batch)} frames: launch {shape}"
    assert shape["instance"] == gpu.INSTANCE_BATCH, msg
    assert shape["split"] == split, msg
    assert shape["min_rays"] == shape["max_rays"] == 64 // split, msg
    assert 1 << shape["max_dup_shift"] == split, msg
    assert shape["waves"] == shape["tiles"] * split, msg


@pytest.mark.parametrize("width,instance", [(2047, gpu.INSTANCE_LONE), (2049, gpu.INSTANCE_LONE_WIDE), (4097, gpu.INSTANCE_BATCH)])
def test_always_picks_the_latency_instance_by_window(exp_ctx, width, instance):
    """ALWAYS: one mask register up to 64 words (a 2047-pixel window from pixel 0), two up to 128, the batch kernel beyond 4096 pixels.  The camera
    is rolled by 90 degrees and looks almost level, so its vanishing point lies far left of the screen: ONE left-right segment whose window is
    the whole screen width."""
    ws = scenes.load_world("proc256")
    fr = scenes.make_frame(ws, width, 320, (40.3, 150.0, 60.2), (2.0, 20.0, 90.0))
    assert waves.frame_windows(fr, width, 320) == [width]
    shape = _launch(exp_ctx, [fr], width, 320, gpu.LATENCY_ALWAYS)
    assert shape["instance"] == instance, f"window {width} pixels ({waves.frame_mask_words(fr, width, 320)} words): launch {shape}"
    if instance != gpu.INSTANCE_BATCH:
        assert shape["waves"] == shape["tiles"] * 64 and shape["max_rays"] == 1 and shape["split"] == 0, shape


@pytest.mark.parametrize("width,height,share", [(640, 480, 1.0), (2560, 1440, 1.0), (3840, 2160, 0.75)])
def test_auto_ray_budget(exp_ctx, width, height, share):
    """AUTO: the latency kernel for launches of at most 12288 rays (tiles x 64), three quarters of that above 2560 x 1440, the batch kernel
    beyond.  A batch just below and one just above the budget (within the smallest frame's tiles of it)."""
    frames = _level_frames(width, height) + _path_frames(width, height)[:3]
    limit = int(LONE_RAYS * share) // 64  # tiles
    step = min(waves.frame_tile_count(f) for f in frames)
    below, n_below = waves.batch_with_tiles(frames, limit - step, limit)
    above, n_above = waves.batch_with_tiles(frames, limit, limit + step)
    shape = _launch(exp_ctx, below, width, height, gpu.LATENCY_AUTO)
    assert shape["instance"] in (gpu.INSTANCE_LONE, gpu.INSTANCE_LONE_WIDE), f"{width}x{height}: {n_below} tiles = {n_below * 64} rays: launch {shape}"
    shape = _launch(exp_ctx, above, width, height, gpu.LATENCY_AUTO)
    assert shape["instance"] == gpu.INSTANCE_BATCH, f"{width}x{height}: {n_above} tiles = {n_above * 64} rays: launch {shape}"
