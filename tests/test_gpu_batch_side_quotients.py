"""-m gpu: the batch kernel's side block with approximate texture quotients (cvx_kernels.h: tex_ends_approx, tex_run<true>, tex_row_fallback).

A lane's side pixels now come out of one of three paths: the certified cheap row on the approximate ends (ordinary lanes, nearly every pixel), the
cheap row on exact ends (lanes that redid their ends behind the rare branch: an end behind the near plane, an operand outside the short division's
range), and the fall-back that recomputes the reference's quotients for a pixel whose row is not certain.  Which path a pixel takes must not be
visible: the product library's raybuffers against the CPU oracle, word for word, as tests/test_gpu_batch_clip_classes.py compares them -- single
frames and launches of full 64-ray waves (tests/waves.py), both walk directions of the element loop, on the procedural world at 64 x 48, the
run-rich stripes world at 320 x 200 and a repeating stripes world (render_repeat_kernel).

Poses: ordinary views; cameras inside the terrain and against a wall (solid voxels cross the near plane: near-clipped ends); far and grazing views
(runs of a fraction of a pixel, where |l'| is large and rows are uncertain)."""
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

PROC, PROC_SIZE = "proc256", (64, 48)
# (position as a fraction of the world's dimensions, euler degrees, lodError)
PROC_POSES = [((0.5, 0.8, 0.5), (20.0, 30.0, 0.0), 1.0), ((0.3, 0.7, 0.6), (-5.0, 200.0, 0.0), 8.0), ((0.5, 0.5, 0.5), (-25.0, 300.0, 0.0), 4.0),
              # inside the terrain / against a wall: low in the world, level and tilted, and just above the ground looking along it
              ((0.5, 0.05, 0.5), (0.0, 45.0, 0.0), 1.0), ((0.41, 0.1, 0.33), (15.0, 170.0, 0.0), 1.0), ((0.2, 0.02, 0.8), (-30.0, 260.0, 10.0), 1.0),
              ((0.52, 0.2, 0.47), (60.0, 10.0, 0.0), 1.0), ((0.52, 0.3, 0.47), (2.0, 95.0, 0.0), 1.0), ((0.7, 0.35, 0.2), (-2.0, 350.0, 0.0), 1.0),
              # far and grazing: high above and outside, looking along the surface
              ((-0.4, 0.9, 0.5), (3.0, 90.0, 0.0), 1.0), ((0.5, 1.3, -0.8), (12.0, 0.0, 0.0), 1.0), ((1.6, 0.75, 1.6), (1.0, 225.0, 0.0), 1.0),
              ((0.5, 1.02, 0.5), (0.5, 130.0, 0.0), 1.0), ((0.1, -0.3, 0.1), (-8.0, 45.0, 0.0), 1.0)]
STRIPES, STRIPES_SIZE = "stripes128x256x128", (320, 200)
STRIPES_POSES = [((64.3, 128.0, 20.2), (0.0, 10.0, 0.0)), ((64.3, 400.0, 64.2), (60.0, 30.0, 0.0)), ((64.3, -120.0, 64.2), (-55.0, 200.0, 0.0)),
                 ((64.3, 100.0, 64.2), (25.0, 77.0, 0.0)), ((5.3, 200.0, 120.2), (-20.0, 135.0, 0.0)),
                 # inside a band / against a wall of bands
                 ((64.5, 128.5, 64.5), (0.0, 0.0, 0.0)), ((64.02, 130.3, 64.97), (10.0, 91.0, 0.0)), ((20.5, 60.5, 100.5), (-40.0, 222.0, 0.0)), ((64.3, 254.0, 20.2), (0.0, 10.0, 0.0)),
                 # far and grazing
                 ((-300.3, 260.0, 64.2), (1.0, 90.0, 0.0)), ((64.3, 128.3, -500.2), (0.2, 0.0, 0.0)), ((400.3, -4.0, 400.2), (-1.0, 225.0, 0.0)), ((64.3, 700.0, 64.2), (80.0, 45.0, 0.0))]
REPEAT, REPEAT_K, REPEAT_SIZE = "stripes64x64x64", 32, (320, 240)
# (offset from the centre of the bounded stand-in in voxels, height, euler degrees)
REPEAT_POSES = [((3.3, -7.2), 62.0, (0.0, 37.0, 0.0)), ((-11.6, 5.3), 2.0, (0.0, 130.0, 0.0)), ((3.3, -7.2), 32.0, (-45.0, 130.0, 0.0)), ((3.3, -7.2), 62.0, (65.0, 37.0, 0.0)),
                # inside a band, against a wall; grazing from just above the slab and from below it
                ((0.5, 0.5), 32.5, (0.0, 0.0, 0.0)), ((7.02, -3.97), 20.3, (5.0, 271.0, 0.0)), ((3.3, -7.2), 64.4, (0.5, 37.0, 0.0)), ((3.3, -7.2), 90.0, (4.0, 10.0, 0.0)),
                ((3.3, -7.2), -6.0, (-3.0, 200.0, 0.0))]


def _groups(kind):
    """(world to upload, repeat?, W, H, [(label, world the oracle renders, frame)])"""
    if kind == "proc":
        ws = scenes.load_world(PROC)
        W, H = PROC_SIZE
        cases = [(f"{PROC} {W}x{H} pos={frac} eul={eul} lodError={lod}", ws, scenes.make_frame(ws, W, H, [frac[i] * ws.dims[i] for i in range(3)], eul, lod)) for frac, eul, lod in PROC_POSES]
        return ws, False, W, H, cases
    if kind == "stripes":
        ws = scenes.load_world(STRIPES)
        W, H = STRIPES_SIZE
        return ws, False, W, H, [(f"stripes {W}x{H} pos={pos} eul={eul}", ws, scenes.make_frame(ws, W, H, pos, eul)) for pos, eul in STRIPES_POSES]
    ws = scenes.load_world(REPEAT)
    wt = R.tile_world(ws, REPEAT_K)
    W, H = REPEAT_SIZE
    c = REPEAT_K * ws.dims[0] / 2.0
    cases = []
    for (ox, oz), y, eul in REPEAT_POSES:
        fr = R.frame(ws, W, H, (c + ox, y, c + oz), eul)
        assert fr.camera.FarClip + 32 <= c - max(abs(ox), abs(oz)), "the camera is too close to the edge of the bounded stand-in"
        cases.append((f"repeat {REPEAT} off=({ox}, {oz}) y={y} eul={eul}", wt, fr))
    return ws, True, W, H, cases


def _compare(label, fr, g, o):
    n_td, n_lr = scenes.used_rows(fr)
    for part, gb, ob, n in (("topdown", g[0], o[0], n_td), ("leftright", g[1], o[1], n_lr)):
        diff = gb[:n] != ob[:n]
        if diff.any():
            rows, cols = np.nonzero(diff)
            raise AssertionError(f"{label}/{part}: {int(diff.sum())} of {diff.size} pixels differ; first at ray {rows[0]} pixel {cols[0]}: "
                                 f"gpu {gb[rows[0], cols[0]]:08x} oracle {ob[rows[0], cols[0]]:08x}")
        assert (gb[n:] == CLEAR).all(), f"{label}/{part}: rows beyond the frame's {n} rays were written"


def _draw_batch_kernel(ctx, fr):
    ctx.enable_counters(False)
    ctx.set_latency_kernel(gpu.LATENCY_NEVER)
    try:
        ctx.clear_raybuffers(0, CLEAR)
        ctx.draw_segments(fr, 0)
    finally:
        ctx.set_latency_kernel(gpu.LATENCY_AUTO)
    return ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN), ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)


@pytest.mark.parametrize("kind", ["proc", "stripes", "repeat"])
def test_side_pixels_bit_exact_on_every_path(kind):
    ws, repeat, W, H, cases = _groups(kind)
    oracles = [O.draw_segments(wo, fr, W, H, clear=CLEAR)[:2] for _, wo, fr in cases]
    directions = {bool(fr.camera.InverseElementIterationDirection) for _, _, fr in cases}
    assert directions == {False, True}, "both walk directions of the element loop must be covered"
    drawn = sum(int((o[0] != CLEAR).sum() + (o[1] != CLEAR).sum()) for o in oracles)
    assert drawn > 0
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        if repeat:
            ctx.set_world_repeat(True)
        ctx.set_resolution(W, H)
        for (label, _, fr), o in zip(cases, oracles):
            _compare(f"{label} [product library, batch kernel, single frame]", fr, _draw_batch_kernel(ctx, fr), o)
        waves.check_full_waves(ctx, [fr for _, _, fr in cases], W, H, f"{kind} {W}x{H} [product library]", oracles=oracles, clear=CLEAR)
    finally:
        ctx.close()
