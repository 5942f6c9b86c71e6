"""-m gpu: the inverted-straddle instance of the batch kernel's frustum clip (cvx_kernels.h, `clipTail` and the dispatch above it).

A wave whose clipping lanes do not all straddle the window the ordinary way (foot of the column below the window, top above it) takes a second
ballot: when every lane sees the column INVERTED at both ends -- foot above the window, top below it, the view of a world column in a segment
whose pixel axis runs against the world's up -- the wave runs the mirror image of the all-straddle instance (clip_min against the upper bound,
clip_max against the lower one, constant flags, the mirrored "window untouched" shortcut); otherwise it runs the general instance as before.
The lanes whose path depends on the wave they sit in are the inverted-straddling lanes of a general-instance wave: on their own they would take
the shortcut, beside another lane they run clip_world_bounds and the reference's projection.

As in tests/test_gpu_batch_uniform_instances.py a single frame never holds such a wave (every ray is copied into all lanes of its wave), so
every group of frames is rendered as single frames AND as one launch of full 64-ray waves (waves.check_full_waves), by the product library with
the batch kernel pinned and by the counting build, every frame against the CPU oracle bit for bit.  The counting build's census
(cvxd_clip_census, include/cpuvox_gpu_diag.h) of the full-wave launches must show, on each kind of world, that the new instance ran, that
the general one ran, and that general-instance waves held inverted-straddling lanes beside others.

Kinds of world: the run-rich stripes world at two sizes (cameras above, below, inside one to three voxels under the top / over the floor, at
the edge: the slab's top or floor comes into the window at a different column for neighbouring rays), the procedural world's scenes and edge
poses, and a small repeating world (render_repeat_kernel), whose oracle is the bounded world made of its copies (tests/repeatworld.py)."""
import os

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

STRIPES = "stripes128x256x128"
STRIPES_POSES = [((64.3, 128.0, 20.2), (0.0, 10.0, 0.0)), ((64.3, 400.0, 64.2), (60.0, 30.0, 0.0)), ((64.3, -120.0, 64.2), (-55.0, 200.0, 0.0)),
                 ((64.3, 100.0, 64.2), (25.0, 77.0, 0.0)), ((5.3, 200.0, 120.2), (-20.0, 135.0, 0.0)), ((0.4, 90.0, 64.2), (5.0, 90.0, 0.0)),
                 # inside the world one to three voxels under its top / over its floor
                 ((64.3, 254.0, 20.2), (0.0, 10.0, 0.0)), ((64.3, 2.0, 64.2), (0.0, 77.0, 0.0)), ((64.3, 255.5, 64.2), (10.0, 200.0, 0.0)), ((10.3, 253.0, 10.2), (5.0, 45.0, 0.0)),
                 # ... looking up and down from there, so that the segments on both sides of the vanishing point hold such columns
                 ((64.3, 253.0, 64.2), (-35.0, 120.0, 0.0)), ((64.3, 3.0, 64.2), (35.0, 300.0, 0.0)), ((30.3, 255.0, 100.2), (50.0, 250.0, 0.0)), ((100.3, 1.0, 30.2), (-50.0, 20.0, 0.0))]
PROC_SCENES = ["proc256_t0_lod8", "proc256_t04_lod8", "proc256_t075_lod8", "proc256_t075_lod1", "proc256_low_lod10", "proc256_up_lod4"]
PROC_EDGES = ["face_x0_in", "face_x0_out", "face_zmax_in", "entry_proc256_from_xmax", "hang_proc256_x-3_y0.5_z0", "y0_proc256", "ydimY_proc256", "yabove_proc256",
              "down_proc256_integer", "up_proc256_integer", "roll90", "yaw45_half_proc256"]
# the repeating world: W repeated forever against the bounded world T of K x K copies, camera near T's centre, far clip short of T's edge
REPEAT, REPEAT_K, REPEAT_SIZE = "stripes64x64x64", 32, (320, 240)
# (offset from T's centre in voxels, height, euler degrees).  A level view has no inverted segment: the inverted straddle needs the vanishing point of
# the world's up near the screen, so the cameras look steeply up or down -- from the middle of the slab (both instances, mixed waves), from under its top
# and over its floor, and from above / below the world (the slab's near face enters the window at a different column for neighbouring rays)
REPEAT_POSES = [((3.3, -7.2), 62.0, (0.0, 37.0, 0.0)), ((-11.6, 5.3), 2.0, (0.0, 130.0, 0.0)),
                ((3.3, -7.2), 32.0, (-80.0, 37.0, 0.0)), ((3.3, -7.2), 32.0, (-45.0, 130.0, 0.0)), ((3.3, -7.2), 62.0, (65.0, 37.0, 0.0)), ((3.3, -7.2), 3.0, (80.0, 130.0, 0.0)),
                ((3.3, -7.2), 90.0, (65.0, 10.0, 0.0)), ((3.3, -7.2), -20.0, (-80.0, 10.0, 0.0))]


def _groups(kind):
    """{(world name, W, H): (world to upload, repeat?, [(label, world the oracle renders, frame)])}: the frames of one kind of world, grouped into
    what one launch can hold."""
    out = {}
    if kind == "stripes":
        ws = scenes.load_world(STRIPES)
        for W, H in ((320, 200), (517, 333)):
            out[(STRIPES, W, H)] = (ws, False, [(f"stripes {W}x{H} pos={pos} eul={eul}", ws, scenes.make_frame(ws, W, H, pos, eul)) for pos, eul in STRIPES_POSES])
    elif kind == "proc":
        for name in PROC_SCENES:
            ws, fr, W, H = scenes.scene_frame(name)
            out.setdefault((scenes.SCENES[name][0], W, H), (ws, False, []))[2].append((name, ws, fr))
        for name in PROC_EDGES:
            e = E.BY_NAME[name]
            assert e.world == "proc256", name
            ws, fr = E.frame(e)
            out.setdefault((e.world, e.width, e.height), (ws, False, []))[2].append((name, ws, fr))
    else:
        ws = scenes.load_world(REPEAT)
        wt = R.tile_world(ws, REPEAT_K)
        W, H = REPEAT_SIZE
        c = REPEAT_K * ws.dims[0] / 2.0
        cases = []
        for (ox, oz), y, eul in REPEAT_POSES:
            fr = R.frame(ws, W, H, (c + ox, y, c + oz), eul)
            assert fr.camera.FarClip + 32 <= c - max(abs(ox), abs(oz)), "the camera is too close to T's edge"
            cases.append((f"repeat {REPEAT} off=({ox}, {oz}) y={y} eul={eul}", wt, fr))
        out[(REPEAT + " repeating", W, H)] = (ws, True, cases)
    return out


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


def _through(library, groups, oracles, counting):
    """Every group through one library, as single frames and as one launch of full waves; returns the census arms of the full-wave launches per
    group (counting build)."""
    arms = {}
    name = "counting build" if counting else "product library"
    gpu.use_library(library)
    ctxs = {}
    try:
        for key, (ws, repeat, cases) in groups.items():
            wname, W, H = key
            if wname not in ctxs:
                ctxs[wname] = gpu.Context(0)
                ctxs[wname].upload_world(ws)
                if repeat:
                    ctxs[wname].set_world_repeat(True)
            ctx = ctxs[wname]
            ctx.set_resolution(W, H)
            for (label, _, fr), o in zip(cases, oracles[key]):
                _compare(f"{label} [{name}, batch kernel, single frame]", fr, _draw_batch_kernel(ctx, fr), o)
            if counting:
                ctx.debug_clip_census(reset=True)
            waves.check_full_waves(ctx, [fr for _, _, fr in cases], W, H, f"{wname} {W}x{H} [{name}]", oracles=oracles[key], clear=CLEAR)
            if counting:
                arms[key] = ctx.debug_clip_census()["arms"]
    finally:
        for ctx in ctxs.values():
            ctx.close()
        gpu.use_library(None)
    return arms


@pytest.mark.parametrize("kind", ["proc", "stripes", "repeat"])
def test_inverted_straddle_instance_bit_exact(kind):
    count_lib = os.path.join(os.path.dirname(gpu.lib_path()), "libcpuvox_gpu_count.so")
    assert os.path.exists(count_lib), "libcpuvox_gpu_count.so not built: run `make -C cpuvox_amd/csrc all` (or __graft_entry__.build())"
    groups = _groups(kind)
    oracles = {key: [O.draw_segments(wo, fr, key[1], key[2], clear=CLEAR)[:2] for _, wo, fr in cases] for key, (_, _, cases) in groups.items()}
    _through(None, groups, oracles, counting=False)
    arms = _through(count_lib, groups, oracles, counting=True)
    for key, a in arms.items():
        print(f"{key} full waves: inverted-straddle instance {a['inverted_straddle']}, general {a['general']}, general with inverted-straddling lanes "
              f"{a['general_mixed']} ({a['general_mixed_lanes']} such lanes)")
    assert sum(a["inverted_straddle"] for a in arms.values()) > 0, f"{kind}: no wave took the inverted-straddle instance of the clip"
    assert sum(a["general"] for a in arms.values()) > 0, f"{kind}: no wave took the general instance of the clip"
    assert sum(a["general_mixed"] for a in arms.values()) > 0, f"{kind}: no wave of the general instance held an inverted-straddling lane beside the others"
    # ... and all three inside one launch, not only across them
    assert any(a["inverted_straddle"] > 0 and a["general"] > 0 and a["general_mixed"] > 0 for a in arms.values()), \
        f"{kind}: no launch took both instances with a mixed wave among them"
