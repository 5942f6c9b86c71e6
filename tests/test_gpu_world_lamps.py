"""GPU: point lights in the bake of the device-resident world (cvx_world_light_lamps).

Every result is compared with the dense model of tests/lampmodel.py (tests/lightmodel.py plus a fractions.Fraction walk per voxel and lamp) on the
numpy volume the world was built from: every level read back with cvx_world_read_level equals the host-built LOD chain of the model's colours,
byte for byte.  The cases where only the device path can go wrong (the per-slab cull and its LDS list of kLampList lamps, walks that leave the
brick) assert what they reach from numpy before they call the device, as tests/limitworlds.py does for the other kernels."""
import os
import re

import numpy as np
import pytest

import lampmodel
import lightmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _brushed, _sphere
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _context, _frames
from test_world_brush_cpu import _pick_world
from test_world_lamps_cpu import random_lamps
from test_world_light_cpu import ALPHA, RGB, model_world, random_params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "libcpuvox_gpu_lightrec.so")  # make variant NAME=lightrec DEFS=-DCVX_LIGHT_RECORDS
K = int(re.search(r"constexpr int kLampList = (\d+);", open(os.path.join(ROOT, "cpuvox_amd", "csrc", "cvx_light.hip")).read()).group(1))
TILE, SLAB = 16, 32


def _light(ctx, p, lamps, level_count=5):
    return ctx.world_light_lamps(p["box_min"], p["box_max"], lampmodel.tuples(lamps), sun_dir=p["sun_dir"], sun_level=p["sun_level"], sun_range=p["sun_range"],
                                 sky_level=p["sky_level"], sky_range=p["sky_range"], floor_level=p["floor_level"], target=p["target"], level_count=level_count)


def _levels(ctx):
    return [ctx.read_level(k)[0] for k in range(6)]


def _world_of(dims, solid):
    x, y, z = np.nonzero(solid)
    colour = np.zeros(dims, dtype=np.uint32)
    colour[x, y, z] = (0xFF | (((x * 7 + y * 13 + z * 29) & 0xFFFFFF) << 8)).astype(np.uint32)
    return colour, model_world(dims, solid, colour)


def _lit_and_checked(ctx, dims, solid, colour, p, lamps, label):
    """One call on the device (all levels refreshed) against the model, all six levels; -> the model's new colours."""
    assert _light(ctx, p, lamps) > 0.0, label
    colour = lampmodel.light(solid, colour, p, lamps)
    want = model_world(dims, solid, colour)
    try:
        _assert_levels(ctx, want, want, 5, label)
    finally:
        want.close()
    return colour


def slab_ranges(solid, p):
    """{(tile x, tile z, slab y): (lo, hi)}: the inclusive voxel range of every tile slab the kernel walks for the call (tests/limitworlds.py:
    light_slab_counts), the range its cull tests the lamps against."""
    lo, hi = lightmodel.clip_box(solid.shape, p["box_min"], p["box_max"])
    out = {}
    for tx in range(lo[0], hi[0], TILE):
        for tz in range(lo[2], hi[2], TILE):
            x1, z1 = min(tx + TILE, hi[0]), min(tz + TILE, hi[2])
            ys = np.nonzero(solid[tx:x1, :, tz:z1].any(axis=(0, 2)))[0]
            if len(ys) == 0:
                continue
            y_lo, y_hi = max(lo[1], int(ys[0])), min(hi[1], int(ys[-1]) + 1)
            for y in range(y_lo, y_hi, SLAB):
                out[(tx, tz, y)] = ((tx, y, tz), (x1 - 1, min(y + SLAB, y_hi) - 1, z1 - 1))
    return out


def reaching(lamps, lo, hi):
    """The lamps whose cube [L - (r - 1), L + (r - 1)] meets the inclusive range lo .. hi."""
    return [l for l in lamps if all(l["pos"][a] + l["radius"] - 1 >= lo[a] and l["pos"][a] - l["radius"] + 1 <= hi[a] for a in range(3))]


# ---- random worlds -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,level_count,seed,calls_seed", [((32, 32, 32), False, 5, 1, 201), ((16, 64, 32), False, 4, 2, 302),
                                                                   ((32, 128, 32), True, 5, 3, 203)])
def test_lit_levels_equal_the_model_on_random_worlds(dims, sparse, level_count, seed, calls_seed):
    """The worlds of the CPU test through the real kernels: 20 random calls with 0 .. 16 lamps each (seeds chosen so that the model alone meets the
    coverage conditions), one after the other on one context.  The coverage conditions come from the model first."""
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    rng = np.random.default_rng(calls_seed)
    calls, lit, shadowed = [], 0, 0
    for k in range(20):
        p = random_params(rng, dims, whole=0.6)
        p = dict(p, sun_level=p["sun_level"] // 2, sky_level=p["sky_level"] // 2, floor_level=p["floor_level"] // 4)   # (room for the lamps below 255)
        lamps = random_lamps(rng, solid, p, 16)
        for l in lamps:   # (most of the wide ones narrowed: the model walks every pair in range)
            if l["radius"] > 24 and rng.random() < 0.85:
                l["radius"] = int(rng.integers(3, 13))
        total, stats = lampmodel.lamp_sum(solid, p, lamps)
        lit, shadowed = lit + stats["lit"], shadowed + stats["shadowed"]
        calls.append((f"call {k}", p, lamps, total))
    assert lit >= 2000 and shadowed >= 300, (lit, shadowed)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for name, p, lamps, total in calls:
            assert _light(ctx, p, lamps, level_count) > 0.0, name
            colour = lampmodel.light(solid, colour, p, lamps, total)
            want = model_world(dims, solid, colour)
            try:
                if min(dims[0], dims[2]) >> 5:
                    _assert_levels(ctx, want, ws, level_count, f"{name}: {p} {lamps}")
                else:  # (a world 16 columns wide has no LOD-5 column to read back: the refreshed levels, which is all there are)
                    for k in range(level_count + 1):
                        blob, count = ctx.read_level(k)
                        assert count == want.info(k).columnCount and blob == want.storage(k).tobytes(), f"{name}: {p} {lamps}: LOD {k} differs"
            finally:
                want.close()
    finally:
        ctx.close()
        ws.close()


def test_no_lamps_equal_world_light_on_a_second_context():
    rng = np.random.default_rng(21)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    p = lightmodel.params((5, 0, 9), (120, 60, 117), sun_dir=(7, 3, -2), sun_level=180, sun_range=300, sky_level=70, sky_range=9, floor_level=5)
    a, b = _context(ws), _context(ws)
    try:
        assert _light(a, p, []) > 0.0
        assert b.world_light(p["box_min"], p["box_max"], sun_dir=p["sun_dir"], sun_level=p["sun_level"], sun_range=p["sun_range"], sky_level=p["sky_level"],
                             sky_range=p["sky_range"], floor_level=p["floor_level"], target=p["target"]) > 0.0
        assert _levels(a) == _levels(b)
    finally:
        a.close()
        b.close()
        ws.close()


# ---- the cull: its list, its boundary ----------------------------------------------------------------------------------------------------------------

CULL_DIMS = (64, 64, 64)


def _cull_world():
    """A floor two voxels thick with a few posts on the tile (16 .. 31, 16 .. 31): that tile has one slab, y = 0 .. 11."""
    solid = np.zeros(CULL_DIMS, dtype=bool)
    solid[:, :2, :] = True
    for x, z in ((18, 19), (25, 22), (29, 30), (21, 27)):
        solid[x, :12, z] = True
    return solid


@pytest.mark.parametrize("count", [K - 1, K, K + 1, 2 * K + 1])
def test_the_cull_list_at_and_past_its_capacity(count):
    """Exactly `count` lamps reach the tile slab (16, 16, 0), more than the LDS list holds from K + 1 on: they are taken in rounds, never dropped.
    Every lamp matters: the model shows for each a voxel of the slab that it lights and that stays below 255.  The same lamps in shuffled order
    give identical bytes."""
    solid = _cull_world()
    colour, ws = _world_of(CULL_DIMS, solid)
    p = lightmodel.params((0, 0, 0), CULL_DIMS, sky_range=0, target=ALPHA)
    rng = np.random.default_rng(1000 + count)
    lamps = []
    while len(lamps) < count:   # in the air just above the floor
        pos = (int(rng.integers(16, 32)), int(rng.integers(2, 4)), int(rng.integers(16, 32)))
        if not solid[pos]:
            lamps.append(lampmodel.lamp(pos, int(rng.integers(3, 5)), int(rng.integers(6, 14))))
    lo, hi = slab_ranges(solid, p)[(16, 16, 0)]
    assert (lo, hi) == ((16, 0, 16), (31, 11, 31)) and len(reaching(lamps, lo, hi)) == count
    total = lampmodel.lamp_sum(solid, p, lamps)[0]
    unsaturated = (total < 255)[16:32, :, 16:32]
    for l in lamps:
        assert ((lampmodel.lamp_sum(solid, p, [l])[0][16:32, :, 16:32] > 0) & unsaturated).any(), l
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        _lit_and_checked(ctx, CULL_DIMS, solid, colour, p, lamps, f"{count} lamps")
        first = _levels(ctx)
        assert _light(ctx, p, [lamps[i] for i in rng.permutation(count)]) > 0.0   # (TO_ALPHA: idempotent)
        assert _levels(ctx) == first, "the lamps' order shows in the result"
    finally:
        ctx.close()
        ws.close()


def test_the_cull_boundary_on_all_six_sides():
    """The box is the tile (16 .. 31, 16 .. 31), its slab y = 0 .. 11.  Six lamps whose cube touches the slab by exactly one voxel, one per side, each
    lighting voxels of it; and six one voxel farther out, whose cube misses it: they must contribute nothing (no voxel is within their radius)."""
    solid = _cull_world()
    solid[20:28, 11, 20:28] = True   # a platform at the slab's top, lit from above
    for x, z in ((16, 24), (31, 24), (24, 16), (24, 31)):   # posts on the tile's edges, lit from the sides
        solid[x, :12, z] = True
    colour, ws = _world_of(CULL_DIMS, solid)
    p = lightmodel.params((16, 0, 16), (32, 64, 32), sky_range=0, target=ALPHA)
    lo, hi = slab_ranges(solid, p)[(16, 16, 0)]
    assert (lo, hi) == ((16, 0, 16), (31, 11, 31))
    r = 8
    touching = [lampmodel.lamp(pos, r, 255) for pos in ((lo[0] + 1 - r, 3, 24), (hi[0] - 1 + r, 3, 24), (24, lo[1] + 1 - r, 23), (24, hi[1] - 1 + r, 24),
                                                       (24, 3, lo[2] + 1 - r), (24, 3, hi[2] - 1 + r))]
    missing = [lampmodel.lamp(pos, r, 255) for pos in ((lo[0] - r, 3, 24), (hi[0] + r, 3, 24), (24, lo[1] - r, 23), (24, hi[1] + r, 24), (24, 3, lo[2] - r),
                                                      (24, 3, hi[2] + r))]
    assert len(reaching(touching, lo, hi)) == 6 and len(reaching(missing, lo, hi)) == 0
    for l in touching:
        assert (lampmodel.lamp_sum(solid, p, [l])[0] > 0).any(), l
    assert not (lampmodel.lamp_sum(solid, p, missing)[0] > 0).any()
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        colour = _lit_and_checked(ctx, CULL_DIMS, solid, colour, p, touching + missing, "touching and missing")
        colour = _lit_and_checked(ctx, CULL_DIMS, solid, colour, dict(p, target=RGB), missing, "missing alone")
    finally:
        ctx.close()
        ws.close()


def test_lamps_outside_the_box_and_the_world_and_a_box_that_cuts_tiles():
    """A box whose edges lie inside tiles, beside a tile without a column; lamps outside the box and outside the world (below, beside, above) shine
    in; skyRange 0 (no halo: every neighbour and walk step beyond the tile comes from the records) and 32 with lamps of radius 64."""
    rng = np.random.default_rng(22)
    solid, _, ws = _pick_world(rng, CULL_DIMS, False)
    ws.close()
    solid[35:53, :, 3:30] = False   # a tile of the box without a column
    colour, ws = _world_of(CULL_DIMS, solid)
    box = ((3, 1, 5), (61, 60, 59))
    assert (35, 5, 1) not in {(k[0], k[1], 1) for k in slab_ranges(solid, lightmodel.params(*box))} and len(slab_ranges(solid, lightmodel.params(*box))) > 12
    lamps = [lampmodel.lamp((-20, 30, 30), 64, 255), lampmodel.lamp((30, -9, 30), 64, 200), lampmodel.lamp((80, 40, 70), 64, 255),
             lampmodel.lamp((30, 70, 30), 64, 255), lampmodel.lamp((1, 20, 2), 30, 180), lampmodel.lamp((62, 25, 62), 40, 255),
             lampmodel.lamp((44, 10, 16), 24, 255), lampmodel.lamp((20, 18, 40), 64, 90)]
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for sky_range in (0, 32):
            p = lightmodel.params(*box, sun_dir=(2, 5, 1), sun_level=60, sun_range=100, sky_level=50, sky_range=sky_range, floor_level=5, target=ALPHA)
            stats = lampmodel.lamp_sum(solid, p, lamps)[1]
            assert stats["lit"] > 2000 and stats["shadowed"] > 2000, stats
            colour = _lit_and_checked(ctx, CULL_DIMS, solid, colour, p, lamps, f"skyRange {sky_range}")
    finally:
        ctx.close()
        ws.close()


def test_a_lamp_64_above_a_slab_walks_on_in_the_records():
    """(32, 128, 32): a floor and a platform at y = 38 .. 39: the tile's second slab starts at y = 32 and its brick holds y = 32 .. 95.  A lamp of
    radius 64 at y = 102 lights the platform 63 below it; the walk leaves the brick's 64 voxels of y -- and, with skyRange 0, the tile's columns --
    and goes on in the records, where a roof fragment at y = 98 .. 99 beside the lamp's column shadows the platform's voxels with x < 8."""
    dims = (32, 128, 32)
    solid = np.zeros(dims, dtype=bool)
    solid[:, :2, :] = True
    solid[4:28, 38:40, 4:28] = True
    solid[13:15, 98:100, 8:20] = True
    colour, ws = _world_of(dims, solid)
    lamps = [lampmodel.lamp((15, 102, 15), 64, 255)]
    box = ((0, 0, 0), (32, 97, 32))   # (the roof itself is not lit: the slabs end below it)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for sky_range in (0, 5):
            p = lightmodel.params(*box, sky_level=40, sky_range=sky_range, target=ALPHA)
            assert (0, 0, 32) in slab_ranges(solid, p)
            total, stats = lampmodel.lamp_sum(solid, p, lamps)
            assert (total[:, 39, :] > 0).sum() > 100 and stats["shadowed"] > 30, stats
            # straight below: 7; ten to either side (d2 = 4069, facing 63 of 73): 1 where lit, 0 behind the roof fragment
            assert total[15, 39, 15] == 255 * (4096 - 3969) // 4096 and total[25, 39, 15] == 255 * 27 * 63 // (4096 * 73) == 1 and total[5, 39, 15] == 0
            colour = _lit_and_checked(ctx, dims, solid, colour, p, lamps, f"skyRange {sky_range}")
    finally:
        ctx.close()
        ws.close()


def test_4096_lamps():
    solid = _cull_world()
    colour, ws = _world_of(CULL_DIMS, solid)
    rng = np.random.default_rng(23)
    lamps = [lampmodel.lamp((int(rng.integers(-2, 66)), int(rng.integers(2, 6)), int(rng.integers(-2, 66))), int(rng.integers(2, 6)), int(rng.integers(20, 80)))
             for _ in range(gpu.LIGHT_MAX_LAMPS)]
    p = lightmodel.params((0, 0, 0), CULL_DIMS, sky_level=30, sky_range=3, floor_level=4, target=RGB)
    most = max(len(reaching(lamps, lo, hi)) for lo, hi in slab_ranges(solid, p).values())
    assert most > K, most   # (some tile slab takes more than one round)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        _lit_and_checked(ctx, CULL_DIMS, solid, colour, p, lamps, "4096 lamps")
    finally:
        ctx.close()
        ws.close()


# ---- determinism, the second implementation, rendering, a sequence, errors ---------------------------------------------------------------------------

def test_two_contexts_give_identical_bytes_and_the_record_walking_variant_agrees():
    rng = np.random.default_rng(24)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    calls = []
    for k in range(2):
        p = lightmodel.params((5, 0, 9), (120, 60, 117), sun_dir=(7, 3, -2), sun_level=90, sun_range=300, sky_level=60, sky_range=(9, 0)[k], floor_level=5,
                              target=(RGB, ALPHA)[k])
        calls.append((p, [l for l in random_lamps(rng, solid, p, 40)] + [lampmodel.lamp((60, 30, 60), 64, 255)]))

    def run():
        ctx = _context(ws)
        try:
            for p, lamps in calls:
                assert _light(ctx, p, lamps) > 0.0
            return _levels(ctx)
        finally:
            ctx.close()

    try:
        first, second = run(), run()
        assert first == second
        if os.path.exists(VARIANT):  # the -DCVX_LIGHT_RECORDS build: every lamp for every voxel, every occupancy test from the records
            gpu.use_library(VARIANT)
            try:
                assert run() == first, "the record-walking variant differs from the product"
            finally:
                gpu.use_library(None)
    finally:
        ws.close()


def test_a_world_lit_with_lamps_renders_like_the_model_world():
    rng = np.random.default_rng(25)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    p = lightmodel.params((0, 0, 0), DIMS, sun_dir=(3, 4, 1), sun_level=70, sun_range=256, sky_level=50, sky_range=6, floor_level=15)
    lamps = [lampmodel.lamp((30, 24, 40), 20, 255), lampmodel.lamp((64, 20, 64), 24, 255), lampmodel.lamp((100, 40, 30), 32, 200),
             lampmodel.lamp((20, 10, 100), 12, 255), lampmodel.lamp((-5, 30, 64), 24, 255)]
    assert lampmodel.lamp_sum(solid, p, lamps)[1]["lit"] > 3000
    want = model_world(DIMS, solid, lampmodel.light(solid, colour, p, lamps))
    ctx = _context(ws)
    try:
        assert _light(ctx, p, lamps) > 0.0
        _assert_levels(ctx, want, want, 5, "lit world")
        _check_world(ctx, want, _frames(want)[:2], "world lit with lamps")
    finally:
        ctx.close()
        ws.close()
        want.close()


def test_a_carved_cave_compacted_and_lit_from_inside():
    rng = np.random.default_rng(26)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    solid2 = solid.copy()
    solid2[30:70, :30, 30:70] = True   # a block of rock to carve into
    colour2, ws2 = _world_of(DIMS, solid2)
    ws.close()
    strokes = [_sphere(gpu.BRUSH_CARVE, (50, 14, 50), 9), _sphere(gpu.BRUSH_CARVE, (58, 14, 52), 6)]
    solid3, colour3 = _brushed(solid2, colour2, strokes)
    p = lightmodel.params((30, 0, 30), (70, 40, 70), sun_dir=(1, 3, 1), sun_level=120, sun_range=200, sky_level=80, sky_range=8, floor_level=6)
    lamps = [lampmodel.lamp((50, 14, 50), 16, 255), lampmodel.lamp((60, 12, 52), 8, 180)]
    total, stats = lampmodel.lamp_sum(solid3, p, lamps)
    without = lightmodel.shades(solid3, p)[1]
    assert stats["lit"] > 500 and (without[total > 0] < 64).all()   # the cave's walls are dim without the lamps
    ctx = _context(ws2)
    try:
        assert ctx.brush(strokes) > 0.0
        ctx.compact()
        _lit_and_checked(ctx, DIMS, solid3, colour3, p, lamps, "the cave")
    finally:
        ctx.close()
        ws2.close()


def test_rejected_calls_leave_the_world_alone():
    rng = np.random.default_rng(27)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    ctx = _context(ws)
    try:
        before = _levels(ctx)
        good = dict(sun_dir=(1, 1, 0), sun_level=100, sun_range=10, sky_level=100, sky_range=4)
        ok = ((5, 5, 5), 8, 200)
        bad = [([ok, ((5, 5, 5), 0, 200)], "radius"), ([ok, ((5, 5, 5), 65, 200)], "radius"), ([((5, 5, 5), 8, 256), ok], "level"), ([((5, 5, 5), 8, -1)], "level"),
               ([ok, ok, ((0, (1 << 20) + 1, 0), 8, 1)], "pos"), ([((-(1 << 20) - 1, 0, 0), 8, 1)], "pos"), ([ok] * 4097, "lampCount")]
        for lamps, match in bad:
            with pytest.raises(gpu.CvxError, match=match):
                ctx.world_light_lamps((0, 0, 0), (8, 8, 8), lamps, **good)
        for kwargs, match in ((dict(good, sky_range=33), "skyRange"), (dict(good, level_count=6), "levelCount")):
            with pytest.raises(gpu.CvxError, match=match):
                ctx.world_light_lamps((0, 0, 0), (8, 8, 8), [ok], **kwargs)
        with pytest.raises(gpu.CvxError, match="boxMin"):
            ctx.world_light_lamps((8, 0, 0), (8, 8, 8), [ok], **good)
        assert _levels(ctx) == before
        # wholly outside the world: CVX_OK, nothing changes, 0 ms
        assert ctx.world_light_lamps((128, 0, 0), (140, 10, 10), [ok], **good) == 0.0
        assert _levels(ctx) == before
    finally:
        ctx.close()
        ws.close()
