"""-m gpu: the wave-uniform instances of the batch kernel's frustum clip (cvx_kernels.h, `clipTail`).  One ballot sends a wave either through
the all-straddle instance (every clipping lane sees the column's foot below and its top above the window at both ends: constant flags, the
"window untouched" shortcut with the reference's path behind a rare branch) or through the general instance (some lane does not straddle:
every lane takes the reference's path, no shortcut test).  The lanes whose path depends on the wave they sit in are the STRADDLING lanes of a
general-instance wave: on their own they would take the shortcut, beside a lane that does not straddle they run the reference's projection
and its window update.

A single frame never holds such a wave: a launch of few tiles is cut into sub-tiles and every ray copied into 2^dupShift lanes (tests/waves.py),
so all lanes of a wave agree.  Every group of frames is therefore rendered as single frames AND as one launch of full 64-ray waves
(waves.check_full_waves: more tiles than half the wave budget, 64 different rays per wave), by the product library with the batch kernel pinned
and by the counting build (`make -C cpuvox_amd/csrc gpu-count`, part of `all`), every frame against the CPU oracle bit for bit.  The counting
build's rows (cvx_debug_section_cycles, include/cpuvox_gpu_diag.h) of the full-wave launches must show, on each kind of world, that both
instances were taken and that general-instance waves held straddling lanes: a lane wrongly treated by its wave's instance is a wrong pixel.

Rows: 13 = wave executions of the all-straddle instance, 14 = of the general instance, 15 = of the general instance with at least one straddling
lane in it ([16 + 15] = those lanes)."""
import os

import numpy as np
import pytest

import edgeposes as E
import oraclelib as O
import scenes
import waves
from cpuvox_amd import gpu

pytestmark = pytest.mark.gpu

CLEAR = E.CLEAR
ROW_ALL_STRADDLE, ROW_GENERAL, ROW_GENERAL_MIXED = 13, 14, 15

STRIPES = "stripes128x256x128"
# cameras above / below the run-rich world (its columns project inside the window: the general instance), inside it (straddling), and at its edge
STRIPES_POSES = [((64.3, 128.0, 20.2), (0.0, 10.0, 0.0)), ((64.3, 400.0, 64.2), (60.0, 30.0, 0.0)), ((64.3, -120.0, 64.2), (-55.0, 200.0, 0.0)),
                 ((64.3, 100.0, 64.2), (25.0, 77.0, 0.0)), ((5.3, 200.0, 120.2), (-20.0, 135.0, 0.0)), ((0.4, 90.0, 64.2), (5.0, 90.0, 0.0)),
                 # ... and inside it one to three voxels under its top / over its floor: the slab [0, dimY] then stops covering a ray's window a few columns
                 # out, at a different step for every ray of a tile -- waves that hold straddling lanes beside others.  (From the middle of this 256-high,
                 # 128-wide world the slab covers the window at every distance inside the world, from outside it never does: those waves agree.)
                 ((64.3, 254.0, 20.2), (0.0, 10.0, 0.0)), ((64.3, 2.0, 64.2), (0.0, 77.0, 0.0)), ((64.3, 255.5, 64.2), (10.0, 200.0, 0.0)), ((10.3, 253.0, 10.2), (5.0, 45.0, 0.0))]
PROC_SCENES = ["proc256_t0_lod8", "proc256_t04_lod8", "proc256_t075_lod8", "proc256_t075_lod1", "proc256_low_lod10", "proc256_up_lod4"]
# edge poses on the procedural world: cameras on a world face (tiles that straddle the world's edge), below / on / above the world (near-clipped columns)
PROC_EDGES = ["face_x0_in", "face_x0_out", "face_zmax_in", "entry_proc256_from_xmax", "hang_proc256_x-3_y0.5_z0", "y0_proc256", "ydimY_proc256", "yabove_proc256",
              "down_proc256_integer", "up_proc256_integer", "roll90", "yaw45_half_proc256"]


def _groups(kind):
    """{(world name, W, H): [(label, world, frame)]}: the frames of one kind of world, grouped into what one launch can hold."""
    out = {}
    if kind == "stripes":
        ws = scenes.load_world(STRIPES)
        for W, H in ((320, 200), (517, 333)):
            for pos, eul in STRIPES_POSES:
                out.setdefault((STRIPES, W, H), []).append((f"stripes {W}x{H} pos={pos} eul={eul}", ws, scenes.make_frame(ws, W, H, pos, eul)))
    else:
        for name in PROC_SCENES:
            ws, fr, W, H = scenes.scene_frame(name)
            out.setdefault((scenes.SCENES[name][0], W, H), []).append((name, ws, fr))
        for name in PROC_EDGES:
            e = E.BY_NAME[name]
            assert e.world == "proc256", name
            ws, fr = E.frame(e)
            out.setdefault((e.world, e.width, e.height), []).append((name, ws, fr))
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
    """Every group through one library, as single frames and as one launch of full waves; returns the count rows of the full-wave launches per
    group (counting build: executions of rows 13, 14, 15 and the lanes of row 15)."""
    rows = {}
    name = "counting build" if counting else "product library"
    gpu.use_library(library)
    ctxs = {}
    try:
        for key, cases in groups.items():
            wname, W, H = key
            if wname not in ctxs:
                ctxs[wname] = gpu.Context(0)
                ctxs[wname].upload_world(cases[0][1])
            ctx = ctxs[wname]
            ctx.set_resolution(W, H)
            for (label, _, fr), o in zip(cases, oracles[key]):
                _compare(f"{label} [{name}, batch kernel, single frame]", fr, _draw_batch_kernel(ctx, fr), o)
            if counting:
                ctx.debug_section_cycles(reset=True)
            waves.check_full_waves(ctx, [fr for _, _, fr in cases], W, H, f"{wname} {W}x{H} [{name}]", oracles=oracles[key], clear=CLEAR)
            if counting:
                c = ctx.debug_section_cycles()
                rows[key] = (int(c[ROW_ALL_STRADDLE]), int(c[ROW_GENERAL]), int(c[ROW_GENERAL_MIXED]), int(c[16 + ROW_GENERAL_MIXED]))
    finally:
        for ctx in ctxs.values():
            ctx.close()
        gpu.use_library(None)
    return rows


@pytest.mark.parametrize("kind", ["proc", "stripes"])
def test_both_clip_instances_bit_exact(kind):
    count_lib = os.path.join(os.path.dirname(gpu.lib_path()), "libcpuvox_gpu_count.so")
    assert os.path.exists(count_lib), "libcpuvox_gpu_count.so not built: run `make -C cpuvox_amd/csrc all` (or __graft_entry__.build())"
    groups = _groups(kind)
    oracles = {key: [O.draw_segments(ws, fr, key[1], key[2], clear=CLEAR)[:2] for _, ws, fr in cases] for key, cases in groups.items()}
    _through(None, groups, oracles, counting=False)
    rows = _through(count_lib, groups, oracles, counting=True)
    for key, r in rows.items():
        print(f"{key} full waves: all-straddle {r[0]}, general {r[1]}, general with straddling lanes {r[2]} ({r[3]} such lanes)")
    assert sum(r[0] for r in rows.values()) > 0, f"{kind}: no wave took the all-straddle instance of the clip"
    assert sum(r[1] for r in rows.values()) > 0, f"{kind}: no wave took the general instance of the clip"
    assert sum(r[2] for r in rows.values()) > 0, f"{kind}: no wave of the general instance held a straddling lane beside the others"
    # ... and all three inside one launch, not only across them
    assert any(r[0] > 0 and r[1] > 0 and r[2] > 0 for r in rows.values()), f"{kind}: no launch took both instances with a mixed wave among them"
