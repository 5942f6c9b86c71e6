"""GPU: finding and filling the enclosed cavities of the device-resident world (cvx_world_cavities).

Every result is compared with the dense model of tests/cavitymodel.py (scipy.ndimage.label on the air of the numpy volume the world was built
from and the brush strokes were applied to): the six totals and the ordered list as exact integers and bytes, each REPORT made twice with
identical bytes.  Every FILL is checked by reading every level back against the host-built LOD chain of the model's result, by rendering through
both kernels against the CPU oracle, and by a second REPORT that selects nothing."""
import ctypes as C

import numpy as np
import pytest

import cavitymodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _box, _brushed, _dense, _world
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _context, _frames
from test_gpu_world_pieces import _serpentine, built  # noqa: F401  (built: the fixture)
from test_world_brush_cpu import _pick_world
from test_world_cavities_cpu import NOISE_DIMS, noise_world, random_call, world_boxes

pytestmark = pytest.mark.gpu

FILL, CARVE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE
REPORT, FILL_CAVITIES = gpu.CAVITIES_REPORT, gpu.CAVITIES_FILL
WHOLE = ((0, 0, 0), DIMS)
ARGB = 0xFF123456
ROCK = 0xFF808080


def _report(ctx, solid, box_min, box_max, open_faces=0x3B, max_voxels=0, capacity=8192, label=""):
    """REPORT twice (identical bytes) against the model: the totals, and the first `capacity` selected cavities byte for byte."""
    want, want_summary, _ = cavitymodel.analyse(solid, box_min, box_max, open_faces, max_voxels)
    got, summary, ms = ctx.world_cavities(box_min, box_max, REPORT, open_faces, max_voxels, capacity=capacity)
    again, summary_again, _ = ctx.world_cavities(box_min, box_max, REPORT, open_faces, max_voxels, capacity=capacity)
    assert summary == want_summary, f"{label}: {summary} != {want_summary}"
    assert len(got) == min(capacity, len(want)), label
    assert got.tobytes() == want[:capacity].tobytes(), f"{label}: first difference at cavity {int(np.argmax(got != want[:capacity]))}"
    assert again.tobytes() == got.tobytes() and summary_again == summary, f"{label}: two calls differ"
    assert ms > 0.0
    return got, summary


def _build(dims, solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def _frames_within(ws, level_count):
    """Two of the edit tests' frames with the LOD distances pushed out so that no ray leaves LOD 0 .. level_count: after a partial refresh the
    levels above still hold the old world (_assert_levels compares them byte for byte), and a world 16 columns wide has no LOD 5 that a mixed
    world set could be built from."""
    frames = _frames(ws)[:2]
    for fr in frames:
        for k in range(level_count, 6):
            fr.camera.LODDistances[k] = 1e9
    return frames


def _fill(ctx, dims, solid, colour, box_min, box_max, open_faces=0x3B, max_voxels=0, level_count=5, argb=ARGB, label=""):
    """FILL on the device against the model: summary and list, every level read back (LOD 0 .. level_count the model's, above as before), a render
    of the refreshed levels through both kernels against the oracle, and a second REPORT that selects nothing.  -> the model's (solid, colour)
    after the fill."""
    want, want_summary, _ = cavitymodel.analyse(solid, box_min, box_max, open_faces, max_voxels)
    assert len(want) > 0, f"{label}: the model selects nothing"
    solid_b, colour_b = cavitymodel.fill(solid, colour, box_min, box_max, open_faces, max_voxels, argb)
    ws_before, ws_after = _build(dims, solid, colour), _build(dims, solid_b, colour_b)
    try:
        got, summary, ms = ctx.world_cavities(box_min, box_max, FILL_CAVITIES, open_faces, max_voxels, argb, level_count, capacity=3)
        assert summary == want_summary and got.tobytes() == want[:3].tobytes() and ms > 0.0, label
        _assert_levels(ctx, ws_after, ws_before, level_count, label)
        visited = _check_world(ctx, ws_after, _frames_within(ws_after, level_count), label)
        assert visited[0] > 0 and not visited[level_count + 1:].any(), f"{label}: levels visited {visited.tolist()}"
        _, after = _report(ctx, solid_b, box_min, box_max, open_faces, max_voxels, label=f"{label}, after the fill")
        assert after["selectedCavities"] == 0 and after["selectedVoxels"] == 0, label
    finally:
        for ws in (ws_before, ws_after):
            ws.close()
    return solid_b, colour_b


# ---- noise worlds --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", NOISE_DIMS)
def test_noise_worlds_report_and_fill(dims):
    """70 % solid noise: more than a thousand cavities, a third of them larger than a voxel.  Whole world, inner box, 40 random calls; then one
    whole-world FILL with levelCount 3 and, on a fresh upload, one inner-box FILL with levelCount 0 and maxVoxels 5."""
    dx, dy, dz = dims
    solid, colour, ws = noise_world(dims)
    want, want_summary, _ = cavitymodel.analyse(solid, (0, 0, 0), dims, 0x3B, 0)
    assert want_summary["enclosedCavities"] >= 100 and int((want["voxels"] > 1).sum()) >= 20, want_summary
    inner = ((3, 2, 5), (dx - 4, dy - 3, dz - 2))
    ctx = _context(ws)
    try:
        _report(ctx, solid, (0, 0, 0), dims, 0x3B, label="whole world")
        _report(ctx, solid, *inner, 0x3F, label="inner box")
        rng = np.random.default_rng(dims[0] + 100)
        for k in range(40):
            box_min, box_max, open_faces, max_voxels = random_call(rng, dims)
            _report(ctx, solid, box_min, box_max, open_faces, max_voxels, capacity=int(rng.choice([0, 3, 8192])), label=f"random call {k}")
        _fill(ctx, dims, solid, colour, (0, 0, 0), dims, 0x3B, 0, 3, label="whole-world FILL")
        ctx.upload_world(ws)
        _fill(ctx, dims, solid, colour, *inner, 0x3F, 5, 0, label="inner-box FILL of the small ones")
    finally:
        ctx.close()
        ws.close()


# ---- the terrain worlds --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((32, 128, 32), True, 3)])
def test_report_equals_the_model_on_terrain_worlds(dims, sparse, seed):
    """Records with 1 .. 3 runs, run-list columns, both colour layouts, empty columns: few or no cavities, but the sky region with a node in every
    column, columns without a node and (sparse) empty columns."""
    rng = np.random.default_rng(seed)
    solid, _, ws = _pick_world(rng, dims, sparse)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for name, (box_min, box_max, open_faces, max_voxels) in world_boxes(dims).items():
            _report(ctx, solid, box_min, box_max, open_faces, max_voxels, label=name)
    finally:
        ctx.close()
        ws.close()


# ---- constructed cases ---------------------------------------------------------------------------------------------------------------------------

def _shell(lo, size=10, argb=0xFF00A0FF):
    """A size^3 box shell with a (size - 2)^3 interior."""
    hi = tuple(v + size for v in lo)
    return [_box(FILL, lo, hi, argb), _box(CARVE, tuple(v + 1 for v in lo), tuple(v - 1 for v in hi))]


def test_shells_holes_and_contacts(built):
    strokes = (_shell((20, 10, 20))                                                     # a closed shell
               + [_box(FILL, (38, 8, 38), (58, 28, 50), ROCK), _box(CARVE, (40, 10, 40), (48, 18, 48)), _box(CARVE, (48, 18, 40), (56, 26, 48))]  # two rooms, edge contact only
               + [_box(FILL, (70, 0, 70), (80, 10, 80), ROCK), _box(CARVE, (71, 0, 71), (79, 9, 79))]   # a shell on y = 0, the floor carved beneath it
               + _shell((90, 5, 90), 20) + _shell((96, 11, 96), 8))                     # nested shells
    ctx, solid, colour = built(strokes)
    cavities, summary = _report(ctx, solid, *WHOLE, label="shells")
    assert summary["enclosedCavities"] == 6 and summary["openRegions"] == 1
    assert cavities["voxels"].tolist() == [512, 512, 512, 576, 18 ** 3 - 8 ** 3, 216]
    assert cavities["seed"].tolist() == [[21, 18, 21], [40, 17, 40], [48, 25, 40], [71, 8, 71], [91, 23, 91], [97, 17, 97]]
    assert (cavities[4]["min"] < cavities[5]["min"]).all() and (cavities[5]["max"] < cavities[4]["max"]).all()  # nested bounding boxes
    # the room on y = 0: with -Y open its air escapes through the bottom of the world
    _, summary = _report(ctx, solid, *WHOLE, 0x3F, label="shells, -Y open")
    assert summary["enclosedCavities"] == 5 and summary["openRegions"] == 2 and summary["openVoxels"] == int((~solid).sum()) - summary["enclosedVoxels"]
    shell_box = ((15, 5, 15), (35, 25, 35))
    # one wall voxel carved: no cavity
    hole = _box(CARVE, (25, 19, 25), (26, 20, 26))
    ctx.brush([hole], 5)
    solid, colour = _brushed(solid, colour, [hole])
    _, summary = _report(ctx, solid, *shell_box, 0x3F, label="shell with a hole")
    assert summary["enclosedCavities"] == 0 and summary["openRegions"] == 1
    # the hole plugged, and a voxel of the shell's top edge carved: the interior meets the outside by an edge only
    edge = [_box(FILL, (25, 19, 25), (26, 20, 26), ROCK), _box(CARVE, (29, 19, 25), (30, 20, 26))]
    ctx.brush(edge, 5)
    solid, colour = _brushed(solid, colour, edge)
    cavities, summary = _report(ctx, solid, *shell_box, 0x3F, label="edge contact")
    assert summary["enclosedCavities"] == 1 and int(cavities[0]["voxels"]) == 512


def test_a_serpentine_tunnel_is_one_cavity(built):
    """The convergence test: a one-voxel tunnel of tens of thousands of steps through a solid 64 x 62 x 64 block; every straight piece of it is
    one node per column, and the labels have to travel its whole length."""
    tunnel = []
    for s in _serpentine(62, 2):
        a, b = s["a"], s["b"]
        tunnel.append(_box(CARVE, (a[0] + 1, a[1], a[2] + 1), (b[0] + 1, b[1], b[2] + 1)))
    strokes = [_box(FILL, (0, 1, 0), (64, 63, 64), ROCK)] + tunnel
    assert len(strokes) <= gpu.BRUSH_MAX_STROKES
    ctx, solid, colour = built(strokes)
    path = int((~solid[0:64, 1:63, 0:64]).sum())
    cavities, summary = _report(ctx, solid, *WHOLE, label="serpentine")
    assert summary["enclosedCavities"] == 1 and int(cavities[0]["voxels"]) == path > 50000
    assert cavities[0]["min"].tolist() == [1, 2, 1] and cavities[0]["max"].tolist() == [63, 61, 62]
    # one end opened to the top
    shaft = _box(CARVE, (1, 61, 1), (2, 63, 2))
    ctx.brush([shaft], 5)
    solid, _ = _brushed(solid, colour, [shaft])
    _, summary = _report(ctx, solid, *WHOLE, label="opened serpentine")
    assert summary["enclosedCavities"] == 0 and summary["openRegions"] == 1


POCKETS = [_box(FILL, (10, 1, 10), (60, 40, 60), ROCK), _box(CARVE, (15, 10, 15), (16, 11, 16)), _box(CARVE, (20, 10, 20), (22, 12, 22)),
           _box(CARVE, (26, 10, 26), (29, 13, 29)), _box(CARVE, (35, 10, 35), (43, 18, 43))]  # sealed pockets of 1, 8, 27 and 512 voxels in rock


def test_sizes_select_what_is_filled(built):
    ctx, solid, colour = built(POCKETS)
    cavities, summary = _report(ctx, solid, *WHOLE, label="pockets")
    assert cavities["voxels"].tolist() == [1, 8, 27, 512]
    cavities, summary = _report(ctx, solid, *WHOLE, max_voxels=8, label="pockets up to 8")
    assert summary["enclosedCavities"] == 4 and summary["enclosedVoxels"] == 548 and summary["selectedCavities"] == 2 and cavities["voxels"].tolist() == [1, 8]
    solid, colour = _fill(ctx, DIMS, solid, colour, *WHOLE, max_voxels=8, label="FILL up to 8")
    assert solid[15, 10, 15] and colour[21, 11, 21] == ARGB and not solid[27, 11, 27]
    cavities, _ = _report(ctx, solid, *WHOLE, label="the other two")
    assert cavities["voxels"].tolist() == [27, 512]


def test_a_box_that_cuts_a_cavity(built):
    """The box ends midway through the 8^3 pocket: open through the cut unless the cut face's bit is cleared; then FILL fills the inner part only."""
    ctx, solid, colour = built(POCKETS)
    box = ((30, 5, 30), (39, 25, 50))  # +X face at x = 39: the pocket spans 35 .. 42
    _, summary = _report(ctx, solid, *box, 0x3F, label="cut, +X open")
    assert summary["enclosedCavities"] == 0 and summary["openRegions"] == 1 and summary["openVoxels"] == 4 * 64
    cavities, summary = _report(ctx, solid, *box, 0x3D, label="cut, +X closed")
    assert summary["enclosedCavities"] == 1 and int(cavities[0]["voxels"]) == 4 * 64 and cavities[0]["max"].tolist() == [39, 18, 43]
    solid, colour = _fill(ctx, DIMS, solid, colour, *box, 0x3D, level_count=2, label="FILL of the inner part")
    assert solid[38, 12, 38] and not solid[39, 12, 38]
    cavities, _ = _report(ctx, solid, *WHOLE, label="the rest of the pocket")
    assert cavities["voxels"].tolist() == [1, 8, 27, 4 * 64]


def test_boxes_inside_rock_solid_columns_and_a_split_column(built):
    ctx, solid, colour = built(POCKETS)
    # strictly inside the block; the 27-pocket touches the box's -X and -Y faces with rock across them; the columns around it are solid over the
    # box's whole y range (no node)
    cavities, summary = _report(ctx, solid, (26, 10, 24), (32, 16, 32), 0x3F, label="inside rock")
    assert summary == {"enclosedCavities": 1, "enclosedVoxels": 27, "selectedCavities": 1, "selectedVoxels": 27, "openRegions": 0, "openVoxels": 0}
    _report(ctx, solid, (25, 10, 25), (30, 13, 30), 0x3F, label="a ring of solid columns around the pocket")
    # a foreign column next to the 8-pocket whose encoding cuts one solid span into two adjacent runs: no node between the halves
    dy = DIMS[1]
    runs = [0xFFFF | ((dy - 30) << 16), 0 | (10 << 16), 10 | (10 << 16), 0xFFFF | (10 << 16)]  # air, y 20 .. 29, y 10 .. 19, air
    blob = np.array([0, len(runs) | (10 << 16), 30, 0, *runs, 0, *[0xFF000000 | k for k in range(20)]], dtype=np.uint32).tobytes()
    ctx.set_columns(0, 22, 20, 1, 1, blob, 1)
    solid = solid.copy()
    solid[22, :, 20] = False
    solid[22, 10:30, 20] = True
    cavities, summary = _report(ctx, solid, *WHOLE, label="split column")
    assert cavities["voxels"].tolist() == [1, 8, 10, 27, 512] and cavities[2]["seed"].tolist() == [22, 9, 20]  # (the air under the column: y 0 .. 9)
    _report(ctx, solid, (18, 8, 18), (26, 32, 24), 0x3F, label="split column, in a box")


def test_a_repeating_world_does_not_wrap():
    solid = np.zeros(DIMS, dtype=bool)
    solid[:, 0, :] = True
    solid[0:6, 1:12, 20:30] = True
    solid[122:128, 1:12, 20:30] = True
    solid[0:4, 4:8, 22:26] = False       # a pocket open through x = 0 ...
    solid[124:128, 4:8, 22:26] = False   # ... and one through x = dimX - 1: in the tiled world they face each other
    colour = _dense(solid)
    ws = _world(solid, colour)
    ctx = _context(ws)
    try:
        ctx.set_world_repeat(True)
        cavities, summary = _report(ctx, solid, *WHOLE, 0x38, label="repeating, X faces closed")
        assert cavities["voxels"].tolist() == [64, 64] and cavities["seed"].tolist() == [[0, 7, 22], [124, 7, 22]]
        _, summary = _report(ctx, solid, *WHOLE, 0x3B, label="repeating, X faces open")
        assert summary["enclosedCavities"] == 0
        _report(ctx, solid, (-10, 0, -10), (10, 64, 40), 0x3A, label="repeating, across the origin")
    finally:
        ctx.close()
        ws.close()


# ---- stamp, fill, carve --------------------------------------------------------------------------------------------------------------------------

def test_stamp_fill_then_carve_shows_a_solid_inside(built):
    cut = _box(CARVE, (24, 5, 15), (26, 25, 35))
    origin, direction = np.array([[25.0, 15.5, 25.5]]), np.array([[-1.0, 0.0, 0.0]])  # from inside the cut towards -X
    ctx, solid, colour = built(_shell((20, 10, 20)))
    _, summary, _ = ctx.world_cavities(*WHOLE, FILL_CAVITIES, argb=ARGB)
    assert summary["selectedCavities"] == 1 and summary["selectedVoxels"] == 512
    ctx.brush([cut], 5)
    vox, face, argb, _ = ctx.pick(origin, direction, 64.0)
    assert vox[0].tolist() == [23, 15, 25] and int(face[0]) == 1 and int(argb[0]) == ARGB
    solid_b, colour_b = _brushed(*cavitymodel.fill(solid, colour, *WHOLE, argb=ARGB), [cut])
    ws = _world(solid_b, colour_b)
    try:
        _assert_levels(ctx, ws, ws, 5, "filled and carved")
    finally:
        ws.close()
    # the unfilled copy: the ray passes through the empty inside to the back wall
    hollow, _, _ = built(_shell((20, 10, 20)) + [cut])
    vox, face, argb, _ = hollow.pick(origin, direction, 64.0)
    assert vox[0].tolist() == [20, 15, 25] and int(argb[0]) != ARGB


# ---- errors and atomicity ------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_leave_the_world_alone(built):
    ctx, solid, colour = built(POCKETS)
    before, _ = ctx.read_level(0)
    bad = [
        (dict(box_min=(0, 0, 0), box_max=(0, 8, 8)), "empty"), (dict(box_min=(9, 0, 0), box_max=(8, 8, 8)), "empty"),
        (dict(box_min=(0, 64, 0), box_max=(8, 70, 8)), "outside the world"), (dict(box_min=(-9, 0, 0), box_max=(0, 8, 8)), "outside the world"),
        (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), open_faces=0x40), "openFaces"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), open_faces=-1), "openFaces"),
        (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), op=2), "op"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), op=-1), "op"),
        (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), max_voxels=-1), "maxVoxels"),
        (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), level_count=6), "levelCount"), (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), level_count=-1), "levelCount"),
        (dict(box_min=(0, 0, 0), box_max=(8, 8, 8), capacity=-1), "cavityCapacity"),
    ]
    for kwargs, match in bad:
        with pytest.raises(gpu.CvxError, match=match):
            ctx.world_cavities(**{"op": FILL_CAVITIES, "argb": ARGB, **kwargs})
    L = gpu.lib()
    p = gpu.CavityParams((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(*DIMS), 0x3B, FILL_CAVITIES, ARGB, 0, 0)
    ms = C.c_float()
    assert L.cvx_world_cavities(ctx._h, None, 5, None, 0, None, C.byref(ms)) == -1          # NULL params
    assert L.cvx_world_cavities(ctx._h, C.byref(p), 5, None, 4, None, C.byref(ms)) == -1    # no list with a capacity above 0
    after, _ = ctx.read_level(0)
    assert after == before, "a rejected call changed LOD 0"
    stats = ctx.edit_stats()
    _, summary = _report(ctx, solid, *WHOLE, label="REPORT")
    assert summary["enclosedCavities"] == 4 and ctx.edit_stats() == stats, "a REPORT touched the arena"
    # a FILL that selects nothing: everything enclosed is larger than the limit inside this box
    _, summary, _ = ctx.world_cavities((30, 5, 30), (50, 25, 50), FILL_CAVITIES, 0x3F, 100, ARGB)
    assert summary["enclosedCavities"] == 1 and summary["selectedCavities"] == 0 and ctx.edit_stats() == stats, "a FILL of nothing touched the arena"
    assert ctx.read_level(0)[0] == before
    fresh = gpu.Context(0)
    try:
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            fresh.world_cavities(*WHOLE)
    finally:
        fresh.close()
