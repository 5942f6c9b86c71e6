"""A catalogue of edge frames: cameras placed where the render arithmetic meets exact values.

Seeded random poses (tests/test_gpu_parity.py, tools/soak.py) never land on an exact value, so they never reach the code both kernels and the oracle
have for those cases: axis-parallel rays (the 1e-7 clamp of tDelta, the world-entry step of a ray that does not move along one axis), starts on grid
planes, exact tMax ties (z steps first), NaN and out-of-range (int)float conversions, projections behind the camera, crossings that equal the far clip
or a LOD distance exactly.  Every frame here is built by the host's own frame setup (scenes.make_frame / host.setup_frame, the reference's path): the
segment data is never edited by hand, since the latency kernel relies on half-conditions that only hold for geometrically consistent frames.

Each entry names the oracle events it must reach (oracle/cvx_oracle.h, orc_events) with a minimum count; tests/test_edge_poses.py checks them, and
tests/test_gpu_edge_poses.py draws every entry through both kernels.
"""
from __future__ import annotations

import json
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

import scenes
from cpuvox_amd import host

CLEAR = 0xDEADBEEF
SKYBOX = 0x191919FF
FIXTURE = os.path.join(scenes.GOLDEN, "edge_poses.json")

_worlds: dict = {}


def load_world(name: str) -> host.WorldSet:
    """scenes.load_world, plus 'terrace64': 64^3, every column solid from y = 0 to a height of 8, 16, 24 or 32 (steps of 8 x 8 columns), so that
    run tops sit on known integer heights; and 'pillars64': 64^3, every third 4 x 4 block of columns solid over the full height, the
    others empty."""
    if name == "pillars64":
        if name not in _worlds:
            x, y, z = np.meshgrid(np.arange(64), np.arange(64), np.arange(64), indexing="ij")
            m = (x // 4 + z // 4) % 3 == 0
            xs, ys, zs = x[m], y[m], z[m]
            argb = (0xFF | ((xs * 4 + 2) << 8) | ((ys * 4) << 16) | ((zs * 4 + 1) << 24)).astype(np.uint32)  # bytes A, R, G, B
            _worlds[name] = host.WorldSet.from_voxels((64, 64, 64), xs, ys, zs, argb)
        return _worlds[name]
    if name != "terrace64":
        return scenes.load_world(name)
    if name not in _worlds:
        x, z = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
        h = 8 + 8 * ((x // 8 + z // 8) % 4)
        xs, ys, zs = [], [], []
        for y in range(32):
            m = y < h
            xs.append(x[m]), ys.append(np.full(int(m.sum()), y)), zs.append(z[m])
        xs, ys, zs = (np.concatenate(v) for v in (xs, ys, zs))
        argb = (0xFF | ((xs * 4 + 1) << 8) | ((ys * 8) << 16) | ((zs * 4 + 3) << 24)).astype(np.uint32)  # bytes A, R, G, B
        _worlds[name] = host.WorldSet.from_voxels((64, 64, 64), xs, ys, zs, argb)
    return _worlds[name]


@dataclass
class Edge:
    name: str
    world: str
    width: int
    height: int
    position: tuple
    euler: tuple
    events: dict                       # orc_events field -> minimum count the oracle's walk must reach
    lod_error: float = 1.0
    far_clip: float | None = None      # replaces SetupLods' far clip
    lod_distances: tuple | None = None  # replaces SetupLods' LOD distances
    tags: tuple = field(default_factory=tuple)  # "repeat": also drawn through the repeat kernels (tests/test_gpu_edge_poses.py)


def _axis(world, pos, yaws=(0.0, 90.0, 180.0, 270.0), pitch=0.0, W=64, H=48, prefix="", **kw):
    return [Edge(f"{prefix}{world}_p{pos[0]}_{pos[1]}_{pos[2]}_pitch{pitch:g}_yaw{y:g}", world, W, H, pos, (pitch, y, 0.0), **kw) for y in yaws]


GRID = {"startOnGrid": 1, "dirClamped": 1}
ENTRY_NAN = {"entrySteps": 1, "entryNonFinite": 1}
STRAIGHT = {"f2iInvalid": 1, "startOnGrid": 1, "dirClamped": 1}

CATALOGUE: list[Edge] = [
    # the family on which the reference's walk never ended: direction (1, 0) from outside, entering on integer z (tMax.z = 0 / 0)
    Edge("hang_proc256_x-3_z0", "proc256", 64, 48, (-3.0, 0.0, 0.0), (0.0, 90.0, 0.0), ENTRY_NAN, tags=("repeat",)),
    Edge("hang_proc256_x-3_y0.5_z0", "proc256", 64, 48, (-3.0, 0.5, 0.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    Edge("hang_proc256_x-3_z5", "proc256", 64, 48, (-3.0, 0.0, 5.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    Edge("hang_proc256_x-3_y10_z0", "proc256", 64, 48, (-3.0, 10.0, 0.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    Edge("hang_proc256_x-3_y40_z128", "proc256", 64, 48, (-3.0, 40.0, 128.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    # the same from the far faces (direction (-1, 0) and (0, -1)) and along z (dir.x = 0: tLast.x = -inf, the reference drew skybox)
    Edge("entry_proc256_from_xmax", "proc256", 64, 48, (260.0, 30.0, 77.0), (0.0, 270.0, 0.0), ENTRY_NAN),
    Edge("entry_proc256_from_zmin", "proc256", 64, 48, (100.0, 30.0, -5.0), (0.0, 0.0, 0.0), ENTRY_NAN),
    Edge("entry_proc256_from_zmin_half", "proc256", 64, 48, (100.5, 30.0, -5.5), (0.0, 0.0, 0.0), ENTRY_NAN),
    Edge("entry_proc256_from_zmax", "proc256", 64, 48, (100.0, 30.0, 300.0), (0.0, 180.0, 0.0), {"entrySteps": 1}),
    Edge("entry_mill256_from_xmin", "mill256", 64, 48, (-20.0, 40.0, 128.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    Edge("entry_mill256_from_zmin_high", "mill256", 96, 64, (128.0, 120.0, -40.0), (15.0, 0.0, 0.0), ENTRY_NAN),
    Edge("entry_wide_world_from_xmin", "proc128x256x64", 64, 48, (-8.0, 60.0, 32.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    Edge("entry_wide_world_from_zmin", "proc128x256x64", 64, 48, (64.0, 60.0, -8.0), (0.0, 0.0, 0.0), ENTRY_NAN),
    # cameras exactly on the world's faces, looking in and out
    Edge("face_x0_in", "proc256", 64, 48, (0.0, 50.0, 100.0), (0.0, 90.0, 0.0), GRID),
    Edge("face_x0_out", "proc256", 64, 48, (0.0, 50.0, 100.0), (10.0, 270.0, 0.0), {"startOnGrid": 1, "ties": 1}),
    # (on the face x = dimX the entry step finds tmin = -0 <= 0 for every ray: the reference draws the whole frame as skybox)
    Edge("face_xmax_in", "proc256", 64, 48, (256.0, 50.0, 100.0), (0.0, 270.0, 0.0), GRID),
    Edge("face_z0_in", "proc256", 64, 48, (100.0, 50.0, 0.0), (0.0, 0.0, 0.0), GRID),
    Edge("face_zmax_in", "proc256", 64, 48, (100.0, 50.0, 256.0), (-10.0, 180.0, 0.0), {"startOnGrid": 1}),
    Edge("face_corner_x0_z0", "mill256", 64, 48, (0.0, 60.0, 0.0), (5.0, 45.0, 0.0), {"startOnGrid": 1, "entrySteps": 0}),
    Edge("face_wide_world_xmax", "proc128x256x64", 64, 48, (128.0, 90.0, 64.0), (20.0, 225.0, 0.0), {"startOnGrid": 1}),
    # axis-parallel rays from inside, integer and half-integer starts, level and steep
    *_axis("proc256", (128.0, 128.0, 128.0), events={"startOnGrid": 1, "clipExact": 1}, tags=("repeat",)),
    *_axis("proc256", (100.5, 60.0, 77.5), pitch=50.0, events={"dirClamped": 1}),
    *_axis("mill256", (128.0, 30.0, 128.0), yaws=(0.0, 90.0), pitch=-35.0, events={"startOnGrid": 1}),
    *_axis("proc128x256x64", (40.0, 100.0, 20.0), yaws=(90.0, 180.0), pitch=0.0, events={"startOnGrid": 1}),
    # straight up / down: every ray's direction is a clamp case, projections degenerate (f2i of NaN and out-of-range quotients)
    Edge("down_proc256_integer", "proc256", 64, 48, (128.0, 128.0, 128.0), (90.0, 0.0, 0.0), {**STRAIGHT, "ties": 1, "projNonOrdinary": 1}, tags=("repeat",)),
    Edge("up_proc256_integer", "proc256", 64, 48, (128.0, 128.0, 128.0), (-90.0, 0.0, 0.0), {**STRAIGHT, "ties": 1, "projNonOrdinary": 1}),
    Edge("down_mill256_half", "mill256", 64, 48, (127.5, 200.0, 100.5), (90.0, 0.0, 0.0), {"dirClamped": 1}),
    Edge("up_wide_world", "proc128x256x64", 48, 64, (64.0, 10.0, 32.0), (-90.0, 90.0, 0.0), STRAIGHT),
    Edge("down_outside_corner", "proc256", 64, 48, (-3.0, 300.0, -3.0), (90.0, 45.0, 0.0), {"entrySteps": 1, "dirClamped": 1, "ties": 1}),
    # pitch 0 (forward.y clamped to +0.001) and the mirrored -0.001 clamp, from grid positions
    Edge("level_clamp_up", "proc256", 64, 48, (64.0, 80.0, 64.0), (0.0, 30.0, 0.0), {"startOnGrid": 1}),
    Edge("level_clamp_down", "proc256", 64, 48, (64.0, 80.0, 64.0), (0.01, 30.0, 0.0), {"startOnGrid": 1}),
    # camera height exactly 0, dimY, above dimY, and exactly on a run's top (terrace heights 8 .. 32) and bottom (y = 0)
    Edge("y0_proc256", "proc256", 64, 48, (90.5, 0.0, 90.5), (-20.0, 60.0, 0.0), {}),
    Edge("ydimY_proc256", "proc256", 64, 48, (90.0, 256.0, 90.0), (30.0, 90.0, 0.0), {"startOnGrid": 1, "f2iInvalid": 1}),
    Edge("yabove_proc256", "proc256", 64, 48, (90.0, 400.0, 90.0), (60.0, 0.0, 0.0), GRID),
    Edge("run_top_terrace", "terrace64", 64, 48, (20.0, 16.0, 20.0), (10.0, 90.0, 0.0), {"startOnGrid": 1, "projNonOrdinary": 1}, tags=("repeat",)),
    Edge("run_top_terrace_yaw45", "terrace64", 64, 48, (4.5, 24.0, 4.5), (0.0, 45.0, 0.0), {"ties": 1}),
    Edge("run_bottom_terrace", "terrace64", 64, 48, (40.0, 0.0, 12.0), (-30.0, 180.0, 0.0), {"startOnGrid": 1, "f2iInvalid": 1, "ties": 1}),
    Edge("ydimY_terrace_down", "terrace64", 64, 48, (32.0, 64.0, 32.0), (90.0, 0.0, 0.0), STRAIGHT),
    # a world of full-height columns (camera on its top, inside a pillar's row, and entering from outside)
    Edge("pillars_top_level", "pillars64", 64, 48, (32.0, 64.0, 32.0), (0.0, 90.0, 0.0), GRID),
    Edge("pillars_down", "pillars64", 64, 48, (32.5, 70.0, 32.5), (60.0, 45.0, 0.0), {"ties": 1}),
    Edge("pillars_outside", "pillars64", 64, 48, (-4.0, 8.0, 16.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    Edge("pillars_outside_z", "pillars64", 64, 48, (2.0, 8.0, -4.0), (0.0, 0.0, 0.0), ENTRY_NAN),
    # roll
    Edge("roll90", "proc256", 64, 48, (128.0, 100.0, 128.0), (20.0, 90.0, 90.0), {"startOnGrid": 1}),
    Edge("roll180", "mill256", 64, 48, (128.0, 60.0, 20.0), (-10.0, 0.0, 180.0), {"startOnGrid": 1}),
    # yaw 45 from half-integer positions: x and z crossings at the same distances (ties, z first)
    Edge("yaw45_half_proc256", "proc256", 64, 48, (100.5, 60.0, 100.5), (20.0, 45.0, 0.0), {"ties": 1}, tags=("repeat",)),
    Edge("yaw45_half_mill256", "mill256", 64, 48, (150.5, 40.0, 150.5), (20.0, 45.0, 0.0), {"ties": 1}),
    Edge("yaw135_half_negative", "proc256", 64, 48, (-10.5, 50.0, 266.5), (10.0, 135.0, 0.0), {"entrySteps": 1}, tags=("repeat",)),
    # far clip and LOD distances exactly equal to crossings of an axis-parallel ray from x.5 (crossings at 0.5, 1.5, ...: exact)
    Edge("farclip_exact", "proc256", 64, 48, (10.5, 40.0, 100.5), (0.0, 90.0, 0.0), {"clipExact": 1}, far_clip=40.5),
    Edge("lod_exact", "proc256", 64, 48, (10.5, 40.0, 100.5), (0.0, 90.0, 0.0), {"clipExact": 1},
         lod_distances=(8.5, 16.5, 32.5, 64.5, 128.5, 1024.0)),
    Edge("lod_far_exact_minus_x", "proc256", 64, 48, (200.5, 40.0, 100.5), (0.0, 270.0, 0.0), {"clipExact": 2},
         lod_distances=(8.5, 16.5, 32.5, 64.5, 128.5, 1024.0), far_clip=150.5),
    # tiny screens, and one window past 2048 pixels (the latency kernel's two-register seen mask)
    Edge("screen_1x1", "proc256", 1, 1, (128.0, 128.0, 128.0), (0.0, 90.0, 0.0), {"startOnGrid": 1}),
    Edge("screen_2x1", "proc256", 2, 1, (-3.0, 0.0, 0.0), (0.0, 90.0, 0.0), ENTRY_NAN),
    Edge("screen_1x64", "mill256", 1, 64, (128.0, 30.0, 128.0), (90.0, 0.0, 0.0), {"dirClamped": 1, "ties": 1, "projNonOrdinary": 1}),
    Edge("screen_3x2", "proc256", 3, 2, (100.5, 60.0, 100.5), (20.0, 45.0, 0.0), {}),
    Edge("screen_2100x24", "proc256", 2100, 24, (-3.0, 40.0, 128.0), (0.0, 90.0, 0.0), {"entrySteps": 1, "startOnGrid": 1}),
]
BY_NAME = {e.name: e for e in CATALOGUE}
assert len(BY_NAME) == len(CATALOGUE), "catalogue names must be unique"


def frame(e: Edge):
    """(world set, frame) of an entry, through the host's frame setup."""
    ws = load_world(e.world)
    if e.far_clip is None and e.lod_distances is None:
        return ws, scenes.make_frame(ws, e.width, e.height, e.position, e.euler, e.lod_error)
    pose = host.camera_pose(e.position, e.euler, e.width, e.height)
    lods, far = host.setup_lods(pose, ws.max_dimension, e.width, e.height, e.lod_error)
    lods = list(e.lod_distances) if e.lod_distances is not None else lods
    far = e.far_clip if e.far_clip is not None else far
    return ws, host.setup_frame(pose, lods, far, e.width, e.height, ws.dims[1], True)


def step_bound(ws) -> int:
    """What the kernels' step guard assumes a bounded-world ray needs at most: dimX + dimZ + 16 column steps."""
    return ws.dims[0] + ws.dims[2] + 16


def region_problems(fr, td, lr, P: int, width: int, height: int, clear: int = CLEAR):
    """The region invariant of tests/test_oracle.py (test_every_pixel_of_every_ray_written_exactly_the_right_region): every pixel of
    [origMin, origMax] of every used ray written with alpha 255, nothing else touched, P equal to the area.  Returns a list of failures."""
    vp = fr.vanishingPointScreenSpace
    rc = [max(0, s.RayCount) for s in fr.segments]

    def rnd(v, hi):
        return int(min(max(np.rint(np.float32(v)), 0), hi))

    bounds = [(rnd(vp[1], height - 1), height - 1), (0, rnd(vp[1], height - 1)), (rnd(vp[0], width - 1), width - 1), (0, rnd(vp[0], width - 1))]
    out, area = [], 0
    for buf, segs in ((td, (0, 1)), (lr, (2, 3))):
        row = 0
        for s in segs:
            lo, hi = bounds[s]
            block = buf[row:row + rc[s]]
            if rc[s]:
                if not (block[:, lo:hi + 1] != clear).all():
                    out.append(f"segment {s}: unwritten pixel inside [origMin, origMax]")
                if not ((block[:, :lo] == clear).all() and (block[:, hi + 1:] == clear).all()):
                    out.append(f"segment {s}: pixel outside the range touched")
                if not ((block[:, lo:hi + 1] & 0xFF) == 0xFF).all():
                    out.append(f"segment {s}: alpha not 255")
                area += rc[s] * (hi - lo + 1)
            row += rc[s]
        if not (buf[row:] == clear).all():
            out.append("rows beyond the used rays touched")
    if P != area:
        out.append(f"P = {P}, area = {area}")
    return out


def crc_pair(fr, td, lr):
    """CRC32 of the used rows of both raybuffers (cleared to 0 where nothing was written: the fixture's convention)."""
    n_td, n_lr = scenes.used_rows(fr)
    return [zlib.crc32(np.ascontiguousarray(td[:n_td]).tobytes()) & 0xFFFFFFFF, zlib.crc32(np.ascontiguousarray(lr[:n_lr]).tobytes()) & 0xFFFFFFFF]


def render_all(names=None):
    """The oracle on every entry (or `names`): name -> {events, counters, region problems, crcs, step bound}.  Used in a child process by the tests
    (a walk that does not end must fail the test, not hang the suite) and by tests/golden/make_edge_poses.py."""
    import oraclelib as O

    out = {}
    for e in CATALOGUE:
        if names is not None and e.name not in names:
            continue
        ws, fr = frame(e)
        td, lr, cnt, ev = O.draw_segments_events(ws, fr, e.width, e.height, clear=CLEAR)
        problems = region_problems(fr, td, lr, cnt.P, e.width, e.height)
        zt, zl = np.where(td == CLEAR, 0, td).astype(np.uint32), np.where(lr == CLEAR, 0, lr).astype(np.uint32)
        out[e.name] = {"events": ev.as_dict(), "counters": cnt.as_dict(), "region": problems, "crcs": crc_pair(fr, zt, zl),
                       "stepBound": step_bound(ws), "rayCounts": [s.RayCount for s in fr.segments]}
    return out


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":  # child-process entry of tests/test_edge_poses.py: the results as one JSON line
    print("RESULT", json.dumps(render_all()))
