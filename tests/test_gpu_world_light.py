"""GPU: sky occlusion and sun shadows baked into the device-resident world (cvx_world_light).

Every result is compared with the dense model of tests/lightmodel.py (padded-array shifts for the sky, a fractions.Fraction walk for the sun) on the
numpy volume the world was built from: every level read back with cvx_world_read_level equals the host-built LOD chain of the model's colours,
byte for byte, and a lit world renders through both kernels what the CPU oracle renders on the model's world."""
import os

import numpy as np
import pytest

import lightmodel
import piecesmodel
import scenes
from cpuvox_amd import gpu, host
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _context, _frames
from test_world_brush_cpu import _pick_world
from test_world_light_cpu import ALPHA, RGB, model_world, random_params, world_calls

pytestmark = pytest.mark.gpu

VARIANT = os.path.join(os.path.dirname(os.path.abspath(gpu.__file__)), "libcpuvox_gpu_lightrec.so")  # make variant NAME=lightrec DEFS=-DCVX_LIGHT_RECORDS


def _light(ctx, p, level_count=5):
    return ctx.world_light(p["box_min"], p["box_max"], sun_dir=p["sun_dir"], sun_level=p["sun_level"], sun_range=p["sun_range"], sky_level=p["sky_level"],
                           sky_range=p["sky_range"], floor_level=p["floor_level"], target=p["target"], level_count=level_count)


def _levels(ctx):
    return [ctx.read_level(k)[0] for k in range(6)]


# ---- random worlds -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,level_count,seed", [((32, 32, 32), False, 5, 1), ((16, 64, 32), False, 4, 2), ((32, 128, 32), True, 5, 3)])
def test_lit_levels_equal_the_model_on_random_worlds(dims, sparse, level_count, seed):
    """The worlds of the CPU test (records with 1 .. 3 runs, run-list columns, both colour layouts) through the real kernels: the named calls and
    40 random parameter sets each (seed = the world's + 100), one after the other on the same context (TO_RGB shades what the call before left)."""
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        rng = np.random.default_rng(seed + 100)
        calls = list(world_calls(dims).items()) + [(f"random parameters {k}", random_params(rng, dims)) for k in range(40)]
        lit = 0
        for name, p in calls:
            ms = _light(ctx, p, level_count)
            mask, _ = lightmodel.shades(solid, p)
            assert ms > 0.0, name
            lit += int(mask.sum())
            colour = lightmodel.light(solid, colour, p)
            want = model_world(dims, solid, colour)
            try:
                if min(dims[0], dims[2]) >> 5:
                    _assert_levels(ctx, want, ws, level_count, f"{name}: {p}")
                else:  # (a world 16 columns wide has no LOD-5 column to read back: the refreshed levels, which is all there are)
                    for k in range(level_count + 1):
                        blob, count = ctx.read_level(k)
                        assert count == want.info(k).columnCount and blob == want.storage(k).tobytes(), f"{name}: {p}: LOD {k} differs"
            finally:
                want.close()
        assert lit > 10000
    finally:
        ctx.close()
        ws.close()


def test_a_partial_refresh_leaves_the_upper_levels():
    rng = np.random.default_rng(11)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    p = lightmodel.params((20, 0, 30), (70, 64, 90), sun_dir=(2, 3, -1), sun_level=150, sun_range=100, sky_level=80, sky_range=5, floor_level=20)
    want = model_world(DIMS, solid, lightmodel.light(solid, colour, p))
    ctx = _context(ws)
    try:
        assert _light(ctx, p, 2) > 0.0
        _assert_levels(ctx, want, ws, 2, "levelCount 2")
    finally:
        ctx.close()
        ws.close()
        want.close()


# ---- the kernel's tiles, slabs and halo ---------------------------------------------------------------------------------------------------------------

def test_a_box_across_many_tiles_and_slabs_with_the_halo_past_the_world():
    """128 x 64 x 128: 8 x 8 tiles of 16 columns and two slabs of 32 voxels; the box's edges lie inside tiles, and with skyRange 8 the halo of the
    outer tiles reaches past the world on all four sides.  Then the same world lit whole with the widest halo."""
    rng = np.random.default_rng(12)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    ctx = _context(ws)
    try:
        for name, p in (("edges inside tiles", lightmodel.params((3, 1, 5), (125, 63, 121), sun_dir=(-3, 2, 5), sun_level=160, sun_range=200, sky_level=95,
                                                                 sky_range=8, target=ALPHA)),
                        ("whole world, skyRange 32", lightmodel.params((-7, -7, -7), (300, 300, 300), sun_dir=(1, 1, 1), sun_level=100, sun_range=4096,
                                                                       sky_level=155, sky_range=32, target=ALPHA)),
                        ("no halo at all", lightmodel.params((0, 0, 0), DIMS, sun_dir=(0, 1, 0), sun_level=255, sun_range=64, sky_range=0, floor_level=0))):
            assert _light(ctx, p) > 0.0
            colour = lightmodel.light(solid, colour, p)
            want = model_world(DIMS, solid, colour)
            try:
                _assert_levels(ctx, want, want, 5, name)
            finally:
                want.close()
    finally:
        ctx.close()
        ws.close()


def test_the_widest_ranges_on_a_tall_world():
    """64 x 256 x 64: eight slabs; skyRange 32 fills the brick's 64 voxels of y, and a steep and a shallow sun with sunRange 4096 leave the brick
    through its top and through its side and go on over the records."""
    dims = (64, 256, 64)
    rng = np.random.default_rng(13)
    solid, colour, ws = _pick_world(rng, dims, False)
    solid2 = solid.copy()
    solid2[20:44, 200:203, 10:50] = True   # a slab high above the terrain: it shadows voxels 150 below it
    x, y, z = np.nonzero(solid2)
    colour2 = np.zeros(dims, dtype=np.uint32)
    colour2[x, y, z] = (0xFF | ((x * 7 + y * 13 + z * 29) << 8)).astype(np.uint32)
    ws.close()
    ws = model_world(dims, solid2, colour2)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        shadowed = 0
        for sun in ((1, 9, 2), (1024, 3, -500), (0, 1, 0)):
            p = lightmodel.params((0, 0, 0), dims, sun_dir=sun, sun_level=200, sun_range=4096, sky_level=55, sky_range=32, target=ALPHA)
            no_walk = dict(p, sun_range=0)
            shadowed += int((lightmodel.shades(solid2, p)[1] != lightmodel.shades(solid2, no_walk)[1]).sum())
            assert _light(ctx, p) > 0.0
            colour2 = lightmodel.light(solid2, colour2, p)
            want = model_world(dims, solid2, colour2)
            try:
                _assert_levels(ctx, want, want, 5, f"sun {sun}")
            finally:
                want.close()
        assert shadowed > 1000
    finally:
        ctx.close()
        ws.close()


# ---- rendering, the mill ---------------------------------------------------------------------------------------------------------------------------------

def test_a_lit_world_renders_like_the_model_world():
    rng = np.random.default_rng(14)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    p = lightmodel.params((0, 0, 0), DIMS, sun_dir=(3, 4, 1), sun_level=150, sun_range=256, sky_level=80, sky_range=6, floor_level=25)
    want = model_world(DIMS, solid, lightmodel.light(solid, colour, p))
    ctx = _context(ws)
    try:
        assert _light(ctx, p) > 0.0
        _assert_levels(ctx, want, want, 5, "lit world")
        _check_world(ctx, want, _frames(want)[:2], "lit world")
    finally:
        ctx.close()
        ws.close()
        want.close()


def test_the_mill_lit_whole():
    fixture = scenes.load_world("mill256")
    dims = tuple(fixture.dims)
    solid, colour = piecesmodel.decode_blob(fixture.storage(0).tobytes(), dims)
    p = lightmodel.params((0, 0, 0), dims, sun_dir=(5, 8, 3), sun_level=140, sun_range=512, sky_level=90, sky_range=6, floor_level=25)
    want = model_world(dims, solid, lightmodel.light(solid, colour, p))
    ctx = _context(fixture)
    try:
        assert _light(ctx, p) > 0.0
        _assert_levels(ctx, want, want, 5, "lit mill")
    finally:
        ctx.close()
        want.close()


# ---- determinism, errors, the second implementation -------------------------------------------------------------------------------------------------

def test_two_contexts_give_identical_bytes_and_the_record_walking_variant_agrees():
    rng = np.random.default_rng(15)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    calls = [lightmodel.params((5, 0, 9), (120, 60, 117), sun_dir=(7, 3, -2), sun_level=180, sun_range=300, sky_level=70, sky_range=9, floor_level=5),
             lightmodel.params((0, 0, 0), DIMS, sun_dir=(-1, 1, 0), sun_level=255, sun_range=4096, sky_level=255, sky_range=3, target=ALPHA)]

    def run():
        ctx = _context(ws)
        try:
            for p in calls:
                assert _light(ctx, p) > 0.0
            return _levels(ctx)
        finally:
            ctx.close()

    try:
        first, second = run(), run()
        assert first == second
        if os.path.exists(VARIANT):  # the -DCVX_LIGHT_RECORDS build: every occupancy test from the records, no brick
            gpu.use_library(VARIANT)
            try:
                assert run() == first, "the record-walking variant differs from the product"
            finally:
                gpu.use_library(None)
    finally:
        ws.close()


def test_rejected_calls_and_boxes_outside_the_world_leave_the_world_alone():
    rng = np.random.default_rng(16)
    solid, colour, ws = _pick_world(rng, DIMS, False)
    ctx = _context(ws)
    try:
        before = _levels(ctx)
        good = dict(sun_dir=(1, 1, 0), sun_level=100, sun_range=10, sky_level=100, sky_range=4)
        bad = [(dict(good, sky_range=33), "skyRange"), (dict(good, sun_range=4097), "sunRange"), (dict(good, sun_level=256), "sunLevel"),
               (dict(good, sky_level=-1), "skyLevel"), (dict(good, floor_level=256), "floorLevel"), (dict(good, target=2), "target"),
               (dict(good, sun_dir=(0, 1025, 0)), "sunDir"), (dict(good, level_count=6), "levelCount"), (dict(good, level_count=-1), "levelCount")]
        for kwargs, match in bad:
            with pytest.raises(gpu.CvxError, match=match):
                ctx.world_light((0, 0, 0), (8, 8, 8), **kwargs)
        with pytest.raises(gpu.CvxError, match="boxMin"):
            ctx.world_light((8, 0, 0), (8, 8, 8), **good)
        assert _levels(ctx) == before
        # wholly outside the world: CVX_OK, nothing changes, 0 ms
        for box in (((128, 0, 0), (140, 10, 10)), ((0, 64, 0), (8, 70, 8)), ((-9, 0, 0), (0, 8, 8))):
            assert ctx.world_light(*box, **good) == 0.0
        assert _levels(ctx) == before
        # a repeating world: coordinates address the stored tile, nothing wraps
        ctx.set_world_repeat(True)
        assert ctx.world_light((128, 0, 0), (140, 10, 10), **good) == 0.0
        assert _levels(ctx) == before
        p = lightmodel.params((-10, 0, -10), (10, 64, 10), target=RGB, **good)
        assert _light(ctx, p) > 0.0
        want = model_world(DIMS, solid, lightmodel.light(solid, colour, p))
        try:
            _assert_levels(ctx, want, want, 5, "repeating world, a box across the origin")
        finally:
            want.close()
    finally:
        ctx.close()
        ws.close()
