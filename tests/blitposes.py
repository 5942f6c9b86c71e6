"""A catalogue of frames for Phase 2 (the blit: blit_kernel, blit_batch_kernel and blit_classify inside the image gather, cvx_kernels.h).

Phase 2 goes wrong where the screen does not divide into 64-pixel tiles, where the seam between two segments runs through pixel centres, where the
vanishing point (VP) sits exactly on the screen centre or tens of thousands of pixels off screen, and where a frame has one segment only.  Every
entry is built by the host's own frame setup (scenes.make_frame / edgeposes.frame); the segment data is never edited by hand.  It holds
  * every entry of edgeposes.CATALOGUE (tiny screens, 2100 x 24, roll 90 / 180, straight up / down, VP far off screen);
  * a VP sweep at 200 x 120: pitch x roll from one camera; with roll 45 the seams are lines y = x + c and pass through pixel centres;
  * seeded random poses at sizes chosen for the tile logic (SIZES);
  * the scenes the blit and image-gather tests of tests/test_gpu_parity.py use, and mill512 at 1080p (GPU only: the oracle takes seconds on it).
tests/test_blit_rule_cpu.py checks the rule itself on the CPU, tests/test_gpu_blit.py the three kernels that apply it; the tags say what an entry
is here for, and has() decides from the frame whether it really has the property."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field

import numpy as np

import edgeposes as E
import scenes

RAY_CLEAR = E.CLEAR          # raybuffers: no voxel colour has it (alpha of every written pixel is 255)
IMAGE_CLEAR = 0xC1EA4000     # numpy images: a second sentinel (alpha 0); the GPU's clear colour is 0
FIXTURE = os.path.join(scenes.GOLDEN, "blit_poses.json")
SEED = 20261016
TAGS = ("partial_width", "partial_height", "seam_through_centres", "vp_far", "vp_centre", "single_segment", "tiny")
TILE = 64                    # CVX_BLIT_TILE; rows per workgroup: 64 (batch blit), 16 (single blit, CVX_BLIT_ROWS_SINGLE)
ROWS_SINGLE = 16

SWEEP_CAMERA = ((128.3, 150.2, 127.9), 33.0)  # position, yaw
SWEEP_PITCH = (90.0, -90.0, 89.999, 45.0, 30.0, 29.0, 20.0, 10.0, 1.0, 0.1, 0.01, 0.0, -0.01, -30.0)
SWEEP_ROLL = (0.0, 45.0, 90.0)
SEAM_FRAMES = {"sweep_pitch30_roll45": 28, "sweep_pitch20_roll45": 9, "sweep_pitch29_roll45": 2}  # pixels no segment claimed before the seam rule
# (W, H, poses): 333 x 217 and 97 x 401 odd both ways; 65 x 17 one pixel past a tile both ways (single blit); 63 x 15 just under one; 129 x 65 the
# same for the batch blit's 64 rows; 1000 x 1 one row; 640 x 360 ten full tile columns, rows 360 = 5 x 64 + 40; 2049 x 70 the latency kernel's
# two-register mask, 33 tile columns and a one-pixel last tile
SIZES = ((333, 217, 4), (97, 401, 4), (65, 17, 4), (63, 15, 4), (129, 65, 4), (1000, 1, 4), (640, 360, 4), (2049, 70, 1))
BLIT_SCENES = ("mill256_t075", "mill256_t09_roll", "proc256_t0_lod8", "proc256_t04_lod8", "proc256_t075_lod8", "proc256_t075_lod1")
GATHER_TIMES = (0.05, 0.3, 0.45, 0.75, 0.9, 1.1, 0.6)  # proc256, 320 x 200, lodError 6: test_image_gather_emulated_on_one_gpu


@dataclass
class Blit:
    name: str
    world: str
    width: int
    height: int
    position: tuple | None      # None: a benchmark-path sample (`path`)
    euler: tuple | None
    lod_error: float = 1.0
    tags: tuple = field(default_factory=tuple)
    edge: E.Edge | None = None  # entry of edgeposes.CATALOGUE (its far clip and LOD distances belong to the frame)
    path: float | None = None   # benchmark clip time
    gpu_only: bool = False


def _size_tags(W, H):
    t = []
    if W % TILE:
        t.append("partial_width")
    if H % TILE and H % ROWS_SINGLE:
        t.append("partial_height")
    if W * H < TILE * ROWS_SINGLE:
        t.append("tiny")
    return t


_EDGE_TAGS = {"down_proc256_integer": ("vp_centre",), "up_proc256_integer": ("vp_centre",), "down_mill256_half": ("vp_centre",),
              "up_wide_world": ("vp_centre",), "down_outside_corner": ("vp_centre",), "ydimY_terrace_down": ("vp_centre",),
              "screen_1x64": ("vp_centre",),
              "level_clamp_up": ("vp_far", "single_segment"), "level_clamp_down": ("vp_far", "single_segment"),
              "hang_proc256_x-3_z0": ("vp_far", "single_segment"), "screen_2100x24": ("vp_far", "single_segment")}


def _build():
    out = []
    for e in E.CATALOGUE:
        out.append(Blit("edge_" + e.name, e.world, e.width, e.height, e.position, e.euler, e.lod_error,
                        tuple(_size_tags(e.width, e.height)) + _EDGE_TAGS.get(e.name, ()), edge=e))
    pos, yaw = SWEEP_CAMERA
    for pitch in SWEEP_PITCH:
        for roll in SWEEP_ROLL:
            name = f"sweep_pitch{pitch:g}_roll{roll:g}"
            tags = _size_tags(200, 120)
            if name in SEAM_FRAMES:
                tags.append("seam_through_centres")
            if abs(pitch) == 90.0:
                tags.append("vp_centre")
            if abs(pitch) <= 0.01:
                tags += ["vp_far", "single_segment"]
            out.append(Blit(name, "proc256", 200, 120, pos, (pitch, yaw, roll), 4.0, tuple(tags)))
    rng = np.random.default_rng(SEED)
    dims = (256, 256, 256)
    for W, H, count in SIZES:
        for i in range(count):
            frac = rng.uniform(-0.2, 1.2, size=3)
            frac[1] = rng.uniform(0.1, 1.1)
            p = tuple(round(float(frac[k] * dims[k]), 3) for k in range(3))
            eul = (round(float(rng.uniform(-89, 89)), 3), round(float(rng.uniform(0, 360)), 3), 0.0 if i % 2 == 0 else round(float(rng.uniform(0, 360)), 3))
            out.append(Blit(f"random_{W}x{H}_{i}", "proc256", W, H, p, eul, 4.0, tuple(_size_tags(W, H))))
    for n in BLIT_SCENES:
        world, W, H, kind, args, lod_error = scenes.SCENES[n]
        assert kind == "path"
        out.append(Blit("scene_" + n, world, W, H, None, None, lod_error, tuple(_size_tags(W, H)), path=args))
    for t in GATHER_TIMES:
        out.append(Blit(f"gather_proc256_t{t:g}", "proc256", 320, 200, None, None, 6.0, tuple(_size_tags(320, 200)), path=t))
    world, W, H, kind, args, lod_error = scenes.SCENES["mill512_t075_1080p"]
    out.append(Blit("scene_mill512_t075_1080p", world, W, H, None, None, lod_error, tuple(_size_tags(W, H)), path=args, gpu_only=True))
    return out


CATALOGUE: list[Blit] = _build()
BY_NAME = {b.name: b for b in CATALOGUE}
assert len(BY_NAME) == len(CATALOGUE), "catalogue names must be unique"
CPU_NAMES = [b.name for b in CATALOGUE if not b.gpu_only]


def frame(b: Blit):
    """(world set, frame) of an entry, through the host's frame setup."""
    if b.edge is not None:
        return E.frame(b.edge)
    ws = E.load_world(b.world)
    if b.path is not None:
        return ws, scenes.benchmark_frame(ws, b.width, b.height, b.path, b.lod_error)
    return ws, scenes.make_frame(ws, b.width, b.height, b.position, b.euler, b.lod_error)


def weights_f64(fr, width, height):
    """Per segment with rays: (s, w[3, H, W]) -- the float64 barycentric weights of oraclelib.blit_reference_f64 (VP, MaxScreen, MinScreen) at every
    pixel centre; segments whose triangle has no area are left out as they are there."""
    ys, xs = np.mgrid[0:height, 0:width]
    cx, cy = xs + 0.5, ys + 0.5
    ax, ay = float(fr.vanishingPointScreenSpace[0]), float(fr.vanishingPointScreenSpace[1])
    out = []
    for s in range(4):
        seg = fr.segments[s]
        if seg.RayCount <= 0:
            continue
        bx, by = float(seg.MaxScreen[0]), float(seg.MaxScreen[1])
        qx, qy = float(seg.MinScreen[0]), float(seg.MinScreen[1])
        area = (bx - ax) * (qy - ay) - (qx - ax) * (by - ay)
        if area == 0.0:
            continue
        w_a = ((bx - cx) * (qy - cy) - (qx - cx) * (by - cy)) / area
        w_b = ((qx - cx) * (ay - cy) - (ax - cx) * (qy - cy)) / area
        out.append((s, np.stack([w_a, w_b, 1.0 - w_a - w_b])))
    return out


def claimed_f64(fr, width, height):
    """Pixels the float64 rule gives to a segment."""
    c = np.zeros((height, width), dtype=bool)
    for _, w in weights_f64(fr, width, height):
        c |= (w >= 0).all(axis=0)
    return c


def has(tag: str, b: Blit, fr, holes_before: int | None = None) -> bool:
    """Whether the frame of an entry really has the property a tag names.  holes_before: pixels the float64 rule claims and the float32 rule
    without the seam rule leaves to no segment (only 'seam_through_centres' needs it)."""
    W, H = b.width, b.height
    vp = [float(v) for v in fr.vanishingPointScreenSpace]
    if tag == "partial_width":
        return W % TILE != 0
    if tag == "partial_height":
        return H % TILE != 0 and H % ROWS_SINGLE != 0
    if tag == "tiny":  # fewer pixels than one tile of the single blit: a seam crosses up to max(W, H) of them, no share of the screen is small
        return W * H < TILE * ROWS_SINGLE
    if tag == "vp_far":
        return max(abs(vp[0]), abs(vp[1])) > 10000.0
    if tag == "vp_centre":  # the centre up to the float32 rounding of the VP: the diagonals then pass within 1e-4 pixels of pixel centres all along
        return abs(vp[0] - W / 2) <= 1e-4 and abs(vp[1] - H / 2) <= 1e-4
    if tag == "single_segment":
        return sum(1 for s in fr.segments if s.RayCount > 0) == 1
    if tag == "seam_through_centres":
        zero = any(((w == 0.0).any(axis=0) & (w >= 0).all(axis=0)).any() for _, w in weights_f64(fr, W, H))
        return zero or bool(holes_before)
    raise KeyError(tag)


def tile_kinds(fr, width, height, rows):
    """The owner test of blit_block (cvx_kernels.h) restated over the float64 weights: for every partial-WIDTH tile of a blit with `rows` rows per
    workgroup, how the kernel treats it -- 'td' (owned by a top / bottom segment: straight stores), 'lr' (owned by a left / right segment: LDS
    gather, then stores) or 'search' (per pixel).  A tile is owned by segment s when at its four corner pixels all weights of s are >= 1e-3 and for
    every earlier segment with rays one and the same weight is <= -1e-3.  Returns the set of kinds the frame's partial-width tiles have."""
    if width % TILE == 0:
        return set()
    ws = weights_f64(fr, width, height)
    x0, x1 = (width // TILE) * TILE, width - 1
    kinds = set()
    for y0 in range(0, height, rows):
        y1 = min(y0 + rows, height) - 1
        owner, earlier_out = -1, True
        for s, w in ws:
            c = w[:, [y0, y0, y1, y1], [x0, x1, x0, x1]]  # [weight, corner]
            if owner < 0 and earlier_out and (c >= 1e-3).all():
                owner = s
            earlier_out = earlier_out and bool((c <= -1e-3).all(axis=1).any())
        kinds.add("search" if owner < 0 else ("td" if owner < 2 else "lr"))
    return kinds


def render_all(names=None):
    """The oracle and both rules on every CPU entry (or `names`): what tests/test_blit_rule_cpu.py asserts and tests/golden/make_blit_poses.py records.
    One oracle render per entry.  Run in a child process by the tests (a walk that does not end must fail the test, not hang the suite)."""
    import oraclelib as O

    out = {}
    for b in CATALOGUE:
        if b.gpu_only or (names is not None and b.name not in names):
            continue
        ws, fr = frame(b)
        W, H = b.width, b.height
        td, lr, _ = O.draw_segments(ws, fr, W, H, clear=RAY_CLEAR, counters=False)
        owner, rays = O.blit_classify_reference(fr, W, H)
        img = O.blit_gather_reference(fr, owner, rays, td, lr, IMAGE_CLEAR)
        before = O.blit_classify_reference(fr, W, H, seam=False)[0]
        img64, margin = O.blit_reference_f64(fr, td, lr, W, H, clear=IMAGE_CLEAR)
        claimed = img64 != IMAGE_CLEAR
        differ = img != img64
        zt, zl = np.where(td == RAY_CLEAR, 0, td).astype(np.uint32), np.where(lr == RAY_CLEAR, 0, lr).astype(np.uint32)
        out[b.name] = {
            "rayCounts": [s.RayCount for s in fr.segments],
            "vp": [float(v) for v in fr.vanishingPointScreenSpace],
            "holes": int(((owner < 0) & claimed).sum()),                  # pixels the float64 rule claims and the float32 rule leaves clear
            "holesBeforeSeamRule": int(((before < 0) & claimed).sum()),
            "claimedBeyondMargin": int(((owner >= 0) & ~claimed & (margin > 1e-4)).sum()),
            "unclaimed": int((owner < 0).sum()),
            "seamRulePixels": int(((before < 0) & (owner >= 0)).sum()),
            "differBeyondMargin": int((differ & (margin > 1e-4)).sum()),
            "differInsideMargin": int((differ & ~(margin > 1e-4)).sum()),
            "pixels": W * H,
            "readsUnwritten": int((img == RAY_CLEAR).sum()),
            "crcImage": scenes.crc(O.blit_gather_reference(fr, owner, rays, zt, zl, 0)),  # the image a GPU makes of raybuffers cleared to 0
            "tags": {t: has(t, b, fr, int(((before < 0) & claimed).sum())) for t in TAGS},
            "tileKinds": {str(rows): sorted(tile_kinds(fr, W, H, rows)) for rows in (ROWS_SINGLE, TILE)},
        }
    return out


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":  # child-process entry of tests/test_blit_rule_cpu.py: the results as one JSON line
    print("RESULT", json.dumps(render_all()))
