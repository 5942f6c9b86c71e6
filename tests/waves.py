"""Full and partial waves of the batch kernel, reached through the product library's own dispatch rule (cvx_gpu.hip DrawBatch).

A launch of few tiles is cut into sub-tiles (split 2, 4, ... 64 while tiles x split x 2 <= CU count x 16), and with the counters off a narrow
sub-tile is widened again by giving every ray 2^dupShift lanes.  A single interactive frame therefore runs one ray per wave, copied into 64
lanes: every wave-wide decision of render_kernel<false> (a ballot, a branch all lanes take together) is uniform by construction.  Only a launch of
more than CU count x 16 / 2 tiles keeps split 1, i.e. 64 different rays in every wave.  The helpers below build such batches out of a caller's
frames (and batches that land on a chosen split factor), and render them with every frame compared against the CPU oracle."""
from __future__ import annotations

import numpy as np

import oraclelib as O
import scenes
from cpuvox_amd import dist, gpu

CLEAR = 0xDEADBEEF
WAVES_PER_CU = 16  # DrawBatch's wave budget: CU count x 16 (cvx_create, splitWaveBudget)
LANES = 64


def cu_count(device: int = 0) -> int:
    import torch

    return torch.cuda.get_device_properties(device).multi_processor_count


def wave_budget(cu: int | None = None) -> int:
    return (cu if cu is not None else cu_count()) * WAVES_PER_CU


def frame_tile_count(frame) -> int:
    """Tiles (64-ray workgroups before any split) the library makes of one frame."""
    return len(dist.frame_tiles([s.RayCount for s in frame.segments]))


def frame_mask_words(frame, width: int, height: int):
    """LDS mask words per lane of every segment that has rays: (omax >> 5) - (omin >> 5) + 1 of its pixel window [origMin, origMax]."""
    ranges = dist.segment_pixel_ranges(frame.vanishingPointScreenSpace, width, height)
    return [(hi >> 5) - (lo >> 5) + 1 for s, (lo, hi) in enumerate(ranges) if frame.segments[s].RayCount > 0]


def frame_windows(frame, width: int, height: int):
    """Pixels of the [origMin, origMax] window of every segment that has rays."""
    ranges = dist.segment_pixel_ranges(frame.vanishingPointScreenSpace, width, height)
    return [hi - lo + 1 for s, (lo, hi) in enumerate(ranges) if frame.segments[s].RayCount > 0]


def expected_split(tiles: int, cu: int | None = None) -> int:
    """DrawBatch's split factor for a launch of `tiles` tiles (counters off or on; CVX_TILE_SPLIT unset)."""
    split, budget = 1, wave_budget(cu)
    while split < LANES and tiles * split * 2 <= budget:
        split *= 2
    return split


def batch_with_tiles(frames, above: int, at_most: int | None, tries: int = 4096):
    """Frames taken from `frames` (cycling, a frame skipped when it would overshoot) until the batch has more than `above` tiles and at most
    `at_most` (None: no bound).  AssertionError if the frames cannot hit the interval."""
    counts = [frame_tile_count(f) for f in frames]
    assert any(counts), "no frame has rays"
    batch, tiles = [], 0
    for i in range(tries):
        k = i % len(frames)
        if counts[k] == 0 or (at_most is not None and tiles + counts[k] > at_most):
            continue
        batch.append(frames[k])
        tiles += counts[k]
        if tiles > above:
            return batch, tiles
    raise AssertionError(f"frames of {counts} tiles do not make a batch of ({above}, {at_most}] tiles")


def full_wave_batch(frames, cu: int | None = None):
    """(batch, buffer_count): the caller's frames repeated (cycling through them) until the launch has more than CU count x 16 / 2 tiles, so
    that DrawBatch keeps split 1 and every wave holds 64 different rays (unless the LDS budget cuts a wide tile).  buffer_count: the raybuffer
    pairs the batch needs (Context(..., buffer_count=...) / Context.set_buffer_count)."""
    batch, _ = batch_with_tiles(frames, wave_budget(cu) // 2, None)
    return batch, len(batch)


def split_batch(frames, split: int, cu: int | None = None):
    """(batch, buffer_count) whose tile count n makes DrawBatch choose `split` (a power of two, 1 .. 64): split doubles while split < 64 and
    n x split x 2 <= budget, so n lies in (budget / (2 split), budget / split] (no upper bound at split 1, no lower one at 64)."""
    assert 1 <= split <= LANES and split & (split - 1) == 0, split
    budget = wave_budget(cu)
    above = budget // (2 * split) if split < LANES else 0
    at_most = budget // split if split > 1 else None
    batch, n = batch_with_tiles(frames, above, at_most)
    assert (split == LANES or n * split * 2 > budget) and (split == 1 or n * split <= budget), (n, split, budget)
    return batch, len(batch)


def oracle(ws, frame, width: int, height: int, clear: int = CLEAR):
    """(top-down, left-right) raybuffers of the CPU oracle, cleared to `clear`."""
    o_td, o_lr, _ = O.draw_segments(ws, frame, width, height, clear=clear, counters=False)
    return o_td, o_lr


def _assert_rows(label, frame, g_td, g_lr, o_td, o_lr, clear):
    n_td, n_lr = scenes.used_rows(frame)
    for part, g, o, n in (("topdown", g_td, o_td, n_td), ("leftright", g_lr, o_lr, n_lr)):
        diff = g[:n] != o[:n]
        if diff.any():
            rows, cols = np.nonzero(diff)
            raise AssertionError(f"{label}/{part}: {int(diff.sum())} of {diff.size} pixels differ; first at ray {rows[0]} pixel {cols[0]}: "
                                 f"gpu {g[rows[0], cols[0]]:08x} oracle {o[rows[0], cols[0]]:08x}; rays affected {len(set(rows.tolist()))}")
        assert (g[n:] == clear).all(), f"{label}/{part}: rows beyond the frame's {n} rays were written"


def check_full_waves(ctx, frames, width: int, height: int, label: str, oracles=None, ws=None, clear: int = CLEAR):
    """Renders full_wave_batch(frames) with the counters off and the batch kernel pinned, in ONE launch, into raybuffers the caller's torch
    tensors hold (cvx_bind_raybuffers).  The first copy of every pose is read back and compared bit for bit with the oracle (`oracles`[k] =
    (top-down, left-right) of frames[k] cleared to `clear`, or computed here from `ws`); every further copy of the pose must equal the first
    on the device.
    The context keeps its world and resolution; its raybuffers are the library's own again afterwards.  Returns the batch's tile count."""
    import torch

    assert ctx.width == width and ctx.height == height
    if oracles is None:
        oracles = [oracle(ws, fr, width, height, clear) for fr in frames]
    keep = [k for k, fr in enumerate(frames) if frame_tile_count(fr) > 0]  # (a frame without rays draws nothing; the batch cycles through the others)
    frames, oracles = [frames[k] for k in keep], [oracles[k] for k in keep]
    batch, buffers = full_wave_batch(frames)
    tiles = sum(frame_tile_count(f) for f in batch)
    label = f"{label} [full waves: {len(batch)} frames, {tiles} tiles in one launch]"
    old = ctx.buffer_count
    assert buffers != old
    ctx.set_buffer_count(buffers)
    try:
        dev = torch.device("cuda", 0)
        lay_td, lay_lr = ctx.raybuffer_layout(gpu.RAYBUFFER_TOPDOWN), ctx.raybuffer_layout(gpu.RAYBUFFER_LEFTRIGHT)
        pools = dist.allocate_pools(buffers, lay_td, lay_lr, dev)
        torch.cuda.synchronize()
        ctx.bind_raybuffers(pools.td.data_ptr(), pools.td.numel() * 4, pools.lr.data_ptr(), pools.lr.numel() * 4)
        for b in range(buffers):
            ctx.clear_raybuffers(b, clear)
        ctx.enable_counters(False)
        ctx.set_latency_kernel(gpu.LATENCY_NEVER)
        try:
            ctx.draw_segments_batch(batch, 0)
        finally:
            ctx.set_latency_kernel(gpu.LATENCY_AUTO)
        td = pools.td.view(buffers, pools.tiles_td, -1)
        lr = pools.lr.view(buffers, pools.tiles_lr, -1)
        for b, fr in enumerate(batch):
            k = b % len(frames)
            if b == k:
                g_td = ctx.read_raybuffer(b, gpu.RAYBUFFER_TOPDOWN)
                g_lr = ctx.read_raybuffer(b, gpu.RAYBUFFER_LEFTRIGHT)
                _assert_rows(f"{label} pose {k}", fr, g_td, g_lr, *oracles[k], clear)
            else:
                for part, pool in (("topdown", td), ("leftright", lr)):
                    if not torch.equal(pool[b], pool[k]):
                        raise AssertionError(f"{label} pose {k}, copy in buffer {b}/{part}: {int((pool[b] != pool[k]).sum())} pixels differ from its first copy")
    finally:
        ctx.set_buffer_count(old)  # (the library's own pools again: the torch tensors go out of scope here)
    return tiles
