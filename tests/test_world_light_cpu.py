"""CPU (no GPU needed): the rules behind cvx_world_light (cpuvox_amd/csrc/cvx_light.h), compiled for the host through tests/light_rules.cpp
(every occupancy test answered from the records), against the independent dense model of tests/lightmodel.py.

- Column mode: 2000 random small worlds (seed 2032) of up to 4 x 4 random columns (records with 1..3 runs and listed columns, both colour
  layouts, foreign encodings with split runs and shared colours) with random boxes (partly outside the world), sun directions (axis-parallel,
  exactly diagonal, near-diagonal, random), all ranges including 0 and the maxima, both targets: every emitted column (runs, colours, worldMin /
  worldMax in the builder's encoding) must equal the model's exactly.
- World mode: small worlds uploaded into a host-only context; the sub-world blob of the call's rectangle equals, byte for byte, the same
  rectangle of the model's world built on the host.
- Constructed cases whose shades are derived by hand and asserted as literals.
- TO_ALPHA twice equals once, TO_RGB with shade 255 is the identity.
- The call without a context / world and every INVALID_ARGUMENT case (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lightmodel
import pyworld
import ruleslib
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world, _random_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RGB, ALPHA = gpu.LIGHT_TO_RGB, gpu.LIGHT_TO_ALPHA


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("light_rules", tmp_path_factory.mktemp("light"))


def random_params(rng, dims, whole=0.3):
    """Random parameters of a call on a world of `dims` (the GPU test uses them too): the box partly outside the world, sun directions of every
    kind, ranges from 0 to the maxima."""
    while True:
        box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
        box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
        if lightmodel.clip_box(dims, box_min, box_max) is not None:
            break
    if rng.random() < whole:
        box_min, box_max = [0, 0, 0], list(dims)
    kind = int(rng.integers(0, 6))
    if kind == 0:
        sun = [0, 0, 0]
        sun[int(rng.integers(0, 3))] = int(rng.choice([-1024, -1, 1, 7, 1024]))
    elif kind == 1:
        sun = [int(v) for v in rng.permutation([1, 1, 0])] if rng.random() < 0.5 else [1, 1, 1]
        sun = [v * int(rng.choice([-1, 1])) * int(rng.choice([1, 5])) if v else 0 for v in sun]
        m = max(abs(v) for v in sun)
        sun = [v // abs(v) * m if v else 0 for v in sun]  # (exactly diagonal: equal magnitudes)
    elif kind == 2:
        sun = [int(v) * int(rng.choice([-1, 1])) for v in rng.permutation([1023, 1024, 1])]
    elif kind == 3:
        sun = [0, 0, 0]
    else:
        sun = [int(rng.integers(-1024, 1025)) if rng.random() < 0.5 else int(rng.integers(-4, 5)) for _ in range(3)]
    return lightmodel.params(box_min, box_max, sun_dir=sun, sun_level=int(rng.choice([0, 255, int(rng.integers(0, 256))])),
                             sun_range=int(rng.choice([0, 1, 4096, int(rng.integers(0, 64))])), sky_level=int(rng.choice([0, 255, int(rng.integers(0, 256))])),
                             sky_range=int(rng.choice([0, 1, 32, int(rng.integers(0, 9))])), floor_level=int(rng.choice([0, 255, int(rng.integers(0, 128))])),
                             target=int(rng.integers(0, 2)))


# ---- column mode -------------------------------------------------------------------------------------------------------------------------------

def _model_case(solid, colour, p):
    lit = lightmodel.light(solid, colour, p)
    gx, dim_y, gz = solid.shape
    columns = []
    for x in range(gx):
        for z in range(gz):
            ys = np.nonzero(solid[x, :, z])[0][::-1]
            col = pyworld.final_column([(int(y), int(lit[x, y, z])) for y in ys], dim_y - 1, 1)
            if col is None:
                columns.append((False, [], [], 0, 0))
                continue
            runs, colours, wmin, wmax = col
            columns.append((False, [((ci & 0xFFFF) | (n << 16)) for ci, n in runs], list(colours), wmin, wmax))
    return columns


def _run_columns(rules, tmp_path, cases):
    words = []
    for dim_y, gx, gz, stride, columns, p in cases:
        words += ruleslib.world_words(dim_y, gx, gz, stride, columns) + lightmodel.words(p)
    out = ruleslib.run_cases(rules, "columns", tmp_path, words)
    results, at = [], 0
    for dim_y, gx, gz, *_ in cases:
        columns, at = ruleslib.edited_columns(out, at, gx * gz)
        results.append(columns)
    assert at == len(out)
    return results


def test_rules_match_the_dense_model_on_random_small_worlds(rules, tmp_path):
    rng = np.random.default_rng(2032)
    cases, models = [], []
    split = shared = listed_like = shadowed = lit = occluded = 0
    for _ in range(2000):
        dim_y = int(rng.choice([8, 16, 64, 256]))
        gx, gz = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        stride = int(rng.choice([1, 32]))
        solid = np.zeros((gx, dim_y, gz), dtype=bool)
        colour = np.zeros((gx, dim_y, gz), dtype=np.uint32)
        columns = []
        for k in range(gx * gz):
            runs, colours, _, dense = _random_column(rng, dim_y)
            x, z = k // gz, k % gz
            colour[x, :, z] = dense
            top = dim_y
            previous_solid = False
            for ci, n in runs:
                if ci >= 0:
                    solid[x, top - n:top, z] = True
                    split += previous_solid
                previous_solid = ci >= 0
                top -= n
            solid_runs = [ci for ci, _ in runs if ci >= 0]
            shared += len(solid_runs) > 1 and all(ci == 0 for ci in solid_runs)
            columns.append((32 + k * 20000 + int(rng.integers(0, 100)), runs, colours))
            listed_like += len(solid_runs) > 3
        colour[~solid] = 0
        p = random_params(rng, (gx, dim_y, gz))
        cases.append((dim_y, gx, gz, stride, columns, p))
        models.append(_model_case(solid, colour, p))
        if any(p["sun_dir"]) and p["sun_level"] == 255 and p["sky_level"] == 0 and p["floor_level"] == 0 and p["target"] == ALPHA:
            mask, shade = lightmodel.shades(solid, p)
            shadowed += int((shade[mask] == 0).sum())
            lit += int((shade[mask] > 0).sum())
        if p["sky_range"] > 0 and p["sky_level"] == 255 and p["sun_level"] == 0 and p["floor_level"] == 0:
            mask, shade = lightmodel.shades(solid, p)
            occluded += int(((shade[mask] > 0) & (shade[mask] < 255)).sum())
    results = _run_columns(rules, tmp_path, cases)
    bad = [i for i, (got, want) in enumerate(zip(results, models)) if got != want]
    if bad:
        i = bad[0]
        k = next(k for k in range(len(models[i])) if results[i][k] != models[i][k])
        raise AssertionError(f"{len(bad)} of {len(cases)} cases differ; first: case {i} {cases[i]}\ncolumn {k}\n got {results[i][k]}\nwant {models[i][k]}")
    assert split > 100 and shared > 100 and listed_like > 300 and shadowed > 200 and lit > 200 and occluded > 500, (split, shared, listed_like, shadowed, lit, occluded)


# ---- world mode ---------------------------------------------------------------------------------------------------------------------------------

def run_world(rules, tmp_path, ws, p, level_count):
    """tests/light_rules.cpp `world` on LOD 0 of ws -> (rectangle, blob bytes, colorShift, listed, over, voxels lit, ms)."""
    info = ws.info(0)
    blob, out = tmp_path / "world.bin", tmp_path / "sub.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                    *[str(v) for v in lightmodel.words(p)], str(level_count), str(out)], text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) over (\d+) rect (\d+) (\d+) (\d+) (\d+) voxels (\d+) ms ([0-9.]+)", text)
    assert m, text
    return (tuple(int(m.group(k)) for k in range(4, 8)), out.read_bytes(), int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(8)), float(m.group(9)))


def model_world(dims, solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=2)


def world_calls(dims):
    """Named parameter sets over a world of `dims` (the GPU test uses them too)."""
    dx, dy, dz = dims
    P = lightmodel.params
    return {
        "whole world, sky and sun": P((0, 0, 0), dims, sun_dir=(3, 5, 2), sun_level=140, sun_range=64, sky_level=90, sky_range=6, floor_level=25),
        "whole world, sky only, alpha": P((0, 0, 0), dims, sky_level=255, sky_range=4, target=ALPHA),
        "inner box, diagonal sun": P((3, 2, 5), (dx - 4, dy - 3, dz - 2), sun_dir=(1, 1, 0), sun_level=200, sun_range=4096, sky_level=40, sky_range=2, floor_level=15),
        "partly outside the world, widest sky": P((-5, -3, dz // 2), (dx // 2, dy + 9, dz + 4), sun_dir=(-1024, 1023, 1), sun_level=255, sun_range=300, sky_level=255,
                                                  sky_range=32, floor_level=0, target=ALPHA),
        "sun from below, no sky": P((0, 0, 0), dims, sun_dir=(0, -1, 0), sun_level=255, sun_range=16, floor_level=3),
        "one column": P((3, 0, 1), (4, dy, 2), sun_dir=(0, 1, 0), sun_level=128, sun_range=8, sky_level=64, sky_range=1, floor_level=64),
    }


@pytest.mark.parametrize("dims,sparse,level_count,seed", [((32, 32, 32), False, 3, 1), ((16, 64, 32), False, 0, 2), ((32, 128, 32), True, 5, 3)])
def test_lit_rectangle_equals_the_model_world(rules, tmp_path, dims, sparse, level_count, seed):
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    nonempty = 0
    try:
        for name, p in world_calls(dims).items():
            rect, got, colour_shift, listed, over, voxels, _ = run_world(rules, tmp_path, ws, p, level_count)
            assert colour_shift == (2 if sparse else 7) and (sparse or listed > 0) and over == 0
            assert rect == lightmodel.rectangle(p, dims, level_count), name
            mask, _ = lightmodel.shades(solid, p)
            assert voxels == int(mask.sum()), name
            nonempty += voxels > 0
            want_ws = model_world(dims, solid, lightmodel.light(solid, colour, p))
            try:
                want, _ = want_ws.extract_region(0, *rect)
            finally:
                want_ws.close()
            assert got == want, f"{name}: the sub-world blob of {rect} differs from the model's ({len(got)} vs {len(want)} bytes)"
    finally:
        ws.close()
    assert nonempty >= 5


# ---- constructed cases: shades derived by hand ----------------------------------------------------------------------------------------------------

def _shade(rules, dims, p, voxels, at):
    """(sky, facing, den, lit, shade) of voxel `at` in a world of the listed solid voxels, from the rules AND from the model (they must agree)."""
    text = subprocess.check_output([rules, "shade", *[str(d) for d in dims], *[str(v) for v in lightmodel.words(p)], str(len(voxels)),
                                    *[str(v) for voxel in voxels for v in voxel], "--", *[str(v) for v in at]], text=True)
    sky, facing, den, lit, shade, through_voxel_shade = [int(v) for v in text.split()]
    assert through_voxel_shade == shade
    solid = np.zeros(dims, dtype=bool)
    for v in voxels:
        solid[tuple(v)] = True
    q = dict(p, box_min=[0, 0, 0], box_max=list(dims))
    mask, model = lightmodel.shades(solid, q)
    assert mask[tuple(at)] and int(model[tuple(at)]) == shade, (int(model[tuple(at)]), shade)
    return sky, facing, den, lit, shade


DIMS = (16, 16, 16)
WHOLE = ((0, 0, 0), DIMS)


def _floor(y=0, thick=1):
    return [(x, y + t, z) for x in range(DIMS[0]) for z in range(DIMS[2]) for t in range(thick)]


def test_a_flat_floor_sees_the_upper_hemisphere(rules):
    """The 8 level directions run along the floor (blocked), the 9 upward ones are open: 9 * 2 = 18; 255 * 18 / 26 = 176."""
    p = lightmodel.params(*WHOLE, sky_level=255, sky_range=4)
    assert _shade(rules, DIMS, p, _floor(), (8, 0, 8)) == (18, 0, 0, 0, 176)
    # the world's edge: outside is air, so the three level directions that leave the world at once are open too: 18 + 3 = 21 -> 255 * 21 / 26 = 205
    assert _shade(rules, DIMS, p, _floor(), (0, 0, 8)) == (21, 0, 0, 0, 205)
    # ... and five of them in a corner: 18 + 5 = 23 -> 225
    assert _shade(rules, DIMS, p, _floor(), (0, 0, 0)) == (23, 0, 0, 0, 225)


def test_a_roof_closer_and_farther_than_the_sky_range(rules):
    roof = [(x, 6, z) for x in range(DIMS[0]) for z in range(DIMS[2])]
    # the roof is 6 above the floor: with skyRange 8 every upward direction ends in it (straight up at s = 6, the slanted ones too): sky 0
    near = lightmodel.params(*WHOLE, sky_level=255, sky_range=8, floor_level=7)
    assert _shade(rules, DIMS, near, _floor() + roof, (8, 0, 8)) == (0, 0, 0, 0, 7)
    # with skyRange 5 no direction reaches it: the floor's 18 -> 7 + 176
    far = lightmodel.params(*WHOLE, sky_level=255, sky_range=5, floor_level=7)
    assert _shade(rules, DIMS, far, _floor() + roof, (8, 0, 8)) == (18, 0, 0, 0, 183)
    # a roof voxel itself: level directions blocked by the roof, upward ones open: 18
    assert _shade(rules, DIMS, far, _floor() + roof, (8, 6, 8))[0] == 18


def test_a_pillar_shadow_along_an_exactly_diagonal_sun(rules):
    """Sun (1, 1, 0): x and y cross their planes at the same parameter and advance together, so the walk from (x, 0, 8) visits (x + k, k, 8) only
    -- never (x + 1, 0, 8) or (x, 1, 8).  A pillar voxel at (9, 3, 8) shadows the floor voxel (6, 0, 8) and no other floor voxel of that row; a
    voxel at (9, 2, 8), which a walk that took the x step before the y step would visit, does not shadow it."""
    p = lightmodel.params(*WHOLE, sun_dir=(1, 1, 0), sun_level=200, sun_range=64)
    pillar = [(9, 3, 8)]
    # facing: +x neighbour (7, 0, 8) is floor (solid), +y neighbour is air: facing 1 of den 2 -> 200 * 1 / 2 = 100 when lit
    assert _shade(rules, DIMS, p, _floor() + pillar, (6, 0, 8)) == (26, 1, 2, 0, 0)
    assert _shade(rules, DIMS, p, _floor() + pillar, (5, 0, 8)) == (26, 1, 2, 1, 100)
    assert _shade(rules, DIMS, p, _floor() + pillar, (7, 0, 8)) == (26, 1, 2, 1, 100)
    assert _shade(rules, DIMS, p, _floor() + [(9, 2, 8)], (6, 0, 8)) == (26, 1, 2, 1, 100)
    # the same along all three axes: (1, 1, 1) from (4, 0, 4) reaches (4 + k, k, 4 + k)
    q = lightmodel.params(*WHOLE, sun_dir=(5, 5, 5), sun_level=240, sun_range=64)
    assert _shade(rules, DIMS, q, _floor() + [(7, 3, 7)], (4, 0, 4)) == (26, 5, 15, 0, 0)
    assert _shade(rules, DIMS, q, _floor() + [(7, 3, 6)], (4, 0, 4)) == (26, 5, 15, 1, 80)
    # a range that ends before the pillar: lit
    short = lightmodel.params(*WHOLE, sun_dir=(1, 1, 0), sun_level=200, sun_range=2)
    assert _shade(rules, DIMS, short, _floor() + pillar, (6, 0, 8)) == (26, 1, 2, 1, 100)
    reaching = lightmodel.params(*WHOLE, sun_dir=(1, 1, 0), sun_level=200, sun_range=3)
    assert _shade(rules, DIMS, reaching, _floor() + pillar, (6, 0, 8)) == (26, 1, 2, 0, 0)


def test_a_sun_straight_below(rules):
    p = lightmodel.params(*WHOLE, sun_dir=(0, -1, 0), sun_level=255, sun_range=16, floor_level=9)
    # the top layer of a two-voxel floor: the voxel below is solid: facing 0, no sun term
    assert _shade(rules, DIMS, p, _floor(0, 2), (8, 1, 8)) == (26, 0, 1, 0, 9)
    # a one-voxel floor at y = 0: the voxel below is outside the world, hence air, and the walk leaves the world at once: the full term
    assert _shade(rules, DIMS, p, _floor(), (8, 0, 8)) == (26, 1, 1, 1, 255)
    # the bottom layer of the two-voxel floor likewise
    assert _shade(rules, DIMS, p, _floor(0, 2), (8, 0, 8)) == (26, 1, 1, 1, 255)


def test_sum_of_terms_saturates_at_255(rules):
    p = lightmodel.params(*WHOLE, sun_dir=(0, 1, 0), sun_level=200, sun_range=16, sky_level=130, sky_range=2, floor_level=30)
    # 30 + 130 * 18 / 26 (= 90) + 200 = 320 -> 255
    assert _shade(rules, DIMS, p, _floor(), (8, 0, 8)) == (18, 1, 1, 1, 255)


# ---- the bake -----------------------------------------------------------------------------------------------------------------------------------------

def test_alpha_twice_equals_once_and_full_shade_is_the_identity():
    rng = np.random.default_rng(5)
    solid, colour, ws = _pick_world(rng, (16, 32, 16), False)
    ws.close()
    colour = np.where(solid, rng.integers(0, 2**32, size=solid.shape, dtype=np.uint64).astype(np.uint32), 0).astype(np.uint32)
    p = lightmodel.params((0, 0, 0), solid.shape, sun_dir=(1, 2, 3), sun_level=120, sun_range=32, sky_level=100, sky_range=3, floor_level=10, target=ALPHA)
    once = lightmodel.light(solid, colour, p)
    assert (lightmodel.light(solid, once, p) == once).all() and (once != colour).any()
    assert ((once & 0xFFFFFF00) == (colour & 0xFFFFFF00)).all()
    full = lightmodel.params((0, 0, 0), solid.shape, floor_level=255, target=RGB)
    assert (lightmodel.light(solid, colour, full) == colour).all()
    half = lightmodel.params((0, 0, 0), solid.shape, floor_level=128, target=RGB)
    lit = lightmodel.light(solid, colour, half)
    assert ((lit & 0xFF) == (colour & 0xFF)).all() and (lit[solid] != colour[solid]).any()  # alpha stays


def test_the_bake_in_the_rules(rules, tmp_path):
    """The same three statements through the header: a one-column world lit with TO_ALPHA, its result lit again; TO_RGB with shade 255."""
    dim_y = 8
    colours = [0x11223344, 0xFFFFFFFF, 0x00000000, 0x80FF7F01]
    column = (32, [(-1, 2), (0, 4), (-1, 2)], colours)

    def run(cols, p):
        return _run_columns(rules, tmp_path, [(dim_y, 1, 1, 1, [(32, [(-1, 2), (0, 4), (-1, 2)], cols)], p)])[0][0]

    p = lightmodel.params((0, 0, 0), (1, dim_y, 1), sky_level=200, sky_range=2, floor_level=11, target=ALPHA)
    once = run(column[2], p)
    # a lone column: every direction leaves the world at once, but straight up (weight 2) is the column itself for all but its top voxel:
    # top 11 + 200 = 211, the others 11 + 200 * 24 / 26 = 195 (colours are listed from the top)
    assert once[2] == [(c & 0xFFFFFF00) | s for c, s in zip(colours, [211, 195, 195, 195])]
    assert run(once[2], p) == once
    assert run(colours, lightmodel.params((0, 0, 0), (1, dim_y, 1), floor_level=255))[2] == colours
    # shade 128 on bytes a r g b = 44 33 22 11 -> alpha stays, (c * 128 + 127) / 255
    assert run(colours, lightmodel.params((0, 0, 0), (1, dim_y, 1), floor_level=128))[2][0] == 0x44 | (((0x33 * 128 + 127) // 255) << 8) | (((0x22 * 128 + 127) // 255) << 16) | (((0x11 * 128 + 127) // 255) << 24)


# ---- layouts and entry points ------------------------------------------------------------------------------------------------------------------

def test_light_fails_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    p = gpu.LightParams()
    p.boxMax[0] = p.boxMax[1] = p.boxMax[2] = 8
    ms = C.c_float()
    assert L.cvx_world_light(None, C.byref(p), 0, C.byref(ms)) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    # a context without a device or world (tests/light_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 21 + [-3, -3], codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_light(h, C.byref(p), 0, C.byref(ms)) == -3
        finally:
            L.cvx_destroy(h)
