"""CPU (no GPU needed): the rules behind cvx_world_spread (cpuvox_amd/csrc/cvx_spread.h), compiled for the host through tests/spread_rules.cpp,
against the independent dense model of tests/spreadmodel.py.  Everything is integers: no comparison has a tolerance.

- The model against itself: the bucketed search and a plain relaxation agree on small boxes, for every mask and both media.
- Noise worlds at about 35 % and 65 % solid uploaded into a host-only context: the host drives the tile relaxation of the kernel one tile after
  the other in a stride-permuted order, and once more in the reversed order; both media, the masks 0x3F, 0x37, 0x3B, horizontal only and one
  direction alone; boxes that stick out of the world; field and totals equal the model's.
- The 66 559-cell serpentine: distances above 32767 and the value 65534 (the working values are unsigned 16 bits), the last 1024 cells unreached.
- The argument check: every rejection with its message, the order of the checks, the boundary values that pass.
- The Python wrappers and the documents (the header's mirrors: tests/test_abi_mirrors.py)."""
import os
import subprocess
import time

import numpy as np
import pytest

import ruleslib
import spreadmodel
from cpuvox_amd import gpu, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AIR, SOLID = gpu.SPREAD_AIR, gpu.SPREAD_SOLID
UNREACHED, BLOCKED = gpu.SPREAD_UNREACHED, gpu.SPREAD_BLOCKED
MASKS = {"all": 0x3F, "water": 0x37, "smoke": 0x3B, "horizontal": 0x33, "+x alone": 0x02}
TOTALS = ("passable", "reached", "largestDistance", "seedsUsed")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("spread_rules", tmp_path_factory.mktemp("spread"))


# ---- worlds the GPU tests share ------------------------------------------------------------------------------------------------------------------

def world_of(solid):
    """A WorldSet of a bool volume (x, y, z), one colour."""
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(solid.shape, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), np.full(len(x), 0xFF6688AA, dtype=np.uint32), threads=2)


def noise_world(seed, dims, share):
    return np.random.default_rng(seed).random(dims) < share


def serpentine(n=64):
    """An n^3 solid world carved into one corridor: every even y layer has full-length x rows at even z, joined by one cell at alternating ends;
    layers are joined by one cell at odd y.  -> (solid, the corridor's cells in order, (x, y, z) each)."""
    solid = np.ones((n, n, n), dtype=bool)
    cells = []
    forward_x, forward_z = True, True
    for y in range(0, n, 2):
        rows = list(range(0, n, 2)) if forward_z else list(range(n - 2, -1, -2))
        for k, z in enumerate(rows):
            xs = range(n) if forward_x else range(n - 1, -1, -1)
            cells.extend((x, y, z) for x in xs)
            last_x = n - 1 if forward_x else 0
            forward_x = not forward_x
            if k + 1 < len(rows):
                cells.append((last_x, y, (z + rows[k + 1]) // 2))
        if y + 2 < n:
            cells.append((cells[-1][0], y + 1, cells[-1][2]))
        forward_z = not forward_z
    c = np.array(cells)
    solid[c[:, 0], c[:, 1], c[:, 2]] = False
    return solid, cells


def seeds_of(rng, dims, count, max_start):
    """`count` seeds anywhere in and a little around the world, starts 0 .. max_start."""
    v = np.stack([rng.integers(-2, d + 2, count) for d in dims], axis=1)
    return [(int(x), int(y), int(z), int(s)) for (x, y, z), s in zip(v, rng.integers(0, max_start + 1, count))]


def same_totals(got, want):
    return {k: got[k] for k in TOTALS} == {k: want[k] for k in TOTALS}


# ---- the model against itself ---------------------------------------------------------------------------------------------------------------------

def test_the_two_models_agree_on_small_boxes():
    rng = np.random.default_rng(3)
    checked = 0
    for share in (0.35, 0.65):
        solid = noise_world(11, (9, 8, 10), share)
        for box in (((0, 0, 0), (9, 8, 10)), ((-2, -1, 3), (5, 10, 12)), ((4, 2, 1), (5, 7, 2))):
            for medium in (AIR, SOLID):
                for mask in MASKS.values():
                    seeds = seeds_of(rng, solid.shape, 5, 3)
                    for cut in (1, 4, 200):
                        seeds_cut = [(x, y, z, min(s, cut)) for x, y, z, s in seeds]
                        got, summary = spreadmodel.field(solid, *box, seeds_cut, medium, mask, cut)
                        want = spreadmodel.slow_field(solid, *box, seeds_cut, medium, mask, cut)
                        assert (got == want).all(), (share, box, medium, mask, cut)
                        assert summary["reached"] == int((want >= 0).sum()) and summary["passable"] == int((want != BLOCKED).sum())
                        checked += 1
    assert checked == 180


def test_the_model_walks_the_serpentine_in_about_a_second():
    solid, cells = serpentine()
    assert len(cells) == 32 * 2079 + 31 == 66559 and len(set(cells)) == len(cells) and int((~solid).sum()) == len(cells)
    assert all(sum(abs(a[i] - b[i]) for i in range(3)) == 1 for a, b in zip(cells, cells[1:])), "a single file"
    t0 = time.perf_counter()
    got, summary = spreadmodel.field(solid, (0, 0, 0), (64, 64, 64), [cells[0] + (0,)], AIR, 0x3F, 65534)
    seconds = time.perf_counter() - t0
    c = np.array(cells)
    along = got[c[:, 0], c[:, 2], c[:, 1]]
    assert (along[:65535] == np.arange(65535)).all() and (along[65535:] == UNREACHED).all() and along.size - 65535 == 1024
    assert summary == {"passable": 66559, "reached": 65535, "largestDistance": 65534, "seedsUsed": 1}
    assert seconds < 20.0, seconds  # (about one second on an idle core; the bound only catches a model that went level by level through numpy)


# ---- the rule header -------------------------------------------------------------------------------------------------------------------------------

def run_fields(rules, tmp_path, ws, queries, env=None):
    """queries: (box_min, box_max, seeds, medium, mask, max_steps, reversed) -> [(field (X, Z, Y), totals dict incl. launches and tileVisits)]."""
    info = ws.info(0)
    blob, src, dst = tmp_path / "world.bin", tmp_path / "queries.bin", tmp_path / "fields.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    words = []
    for lo, hi, seeds, medium, mask, cut, order in queries:
        words += [*lo, *[hi[a] - lo[a] for a in range(3)], medium, mask, cut, int(order), len(seeds)]
        for s in seeds:
            words += [s[0], s[1], s[2], s[3] if len(s) == 4 else 0]
    src.write_bytes(np.array(words, dtype=np.int32).tobytes())
    subprocess.check_call([rules, "fields", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(src), str(dst)], env=env)
    raw = np.frombuffer(dst.read_bytes(), dtype=np.int32)
    out, at = [], 0
    for lo, hi, *_ in queries:
        shape = (hi[0] - lo[0], hi[2] - lo[2], hi[1] - lo[1])
        n = shape[0] * shape[1] * shape[2]
        totals = dict(zip(TOTALS + ("launches", "tileVisits"), raw[at + n:at + n + 6].tolist()))
        out.append((raw[at:at + n].reshape(shape), totals))
        at += n + 6
    assert at == raw.size
    return out


@pytest.mark.parametrize("share", [0.35, 0.65])
def test_tile_relaxation_matches_the_model_in_both_orders(rules, tmp_path, share):
    dims = (32, 128, 16)
    T = gpu.SPREAD_TILE
    boxes = (((0, 0, 0), dims), ((-3, -2, -1), (35, 131, 18)), ((5, 60, 2), (14, 70, 15)))
    sizes = [hi[a] - lo[a] for lo, hi in boxes[1:2] for a in range(3)]
    assert all(sizes[a] % T[a] != 0 and sizes[a] > T[a] for a in range(3)), "several tiles per axis, the last of them not whole"
    solid = noise_world(21 + int(share * 100), dims, share)
    assert abs(solid.mean() - share) < 0.02
    rng = np.random.default_rng(8)
    queries = []
    for box in boxes:
        for medium in (AIR, SOLID):
            for mask in MASKS.values():
                seeds = seeds_of(rng, dims, 7, 5)
                queries += [box + (seeds, medium, mask, 60, order) for order in (False, True)]
    ws = world_of(solid)
    try:
        results = run_fields(rules, tmp_path, ws, queries)
    finally:
        ws.close()
    reached = unreached = several = 0
    for (lo, hi, seeds, medium, mask, cut, order), (got, totals) in zip(queries, results):
        want, summary = spreadmodel.field(solid, lo, hi, seeds, medium, mask, cut)
        bad = got != want
        assert not bad.any(), f"medium {medium} mask {mask:#x} box {lo} .. {hi} reversed {order}: {int(bad.sum())} of {bad.size} differ, first at " \
                              f"{np.argwhere(bad)[0].tolist()} (x, z, y): {got[bad][0]} for {want[bad][0]}"
        assert same_totals(totals, summary), (totals, summary)
        assert 1 <= totals["launches"] <= cut + 2
        reached += summary["reached"]
        unreached += summary["passable"] - summary["reached"]
        several += totals["launches"] > 2
    assert reached > 10000 and unreached > 10000 and several > 10, (reached, unreached, several)


def test_the_serpentine_needs_unsigned_sixteen_bits(rules, tmp_path):
    solid, cells = serpentine()
    ws = world_of(solid)
    try:
        (air, air_totals), (rock, rock_totals) = run_fields(rules, tmp_path, ws, [
            ((0, 0, 0), (64, 64, 64), [cells[0] + (0,)], AIR, 0x3F, 65534, False),
            ((0, 0, 0), (64, 64, 64), [(1, 1, 1, 0)], SOLID, 0x3F, 65534, True)])
    finally:
        ws.close()
    want, summary = spreadmodel.field(solid, (0, 0, 0), (64, 64, 64), [cells[0] + (0,)], AIR, 0x3F, 65534)
    assert int((want > 32767).sum()) == 32767 and int((want == 65534).sum()) == 1 and int((want == UNREACHED).sum()) == 1024
    assert (air == want).all() and same_totals(air_totals, summary) and air_totals["launches"] <= 65536
    want, summary = spreadmodel.field(solid, (0, 0, 0), (64, 64, 64), [(1, 1, 1, 0)], SOLID, 0x3F, 65534)
    assert solid[1, 1, 1] and int((want == BLOCKED).sum()) == 66559 and summary["reached"] == 64 ** 3 - 66559, "one blocked corridor, all around it passable"
    assert (rock == want).all() and same_totals(rock_totals, summary)


def test_the_rules_are_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python) built with -fsanitize=address,undefined: the argument checks and
    a small field in both orders run to the end, and the field is still the model's."""
    out = ruleslib.build("spread_rules", tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (the HIP runtime the library links keeps its own allocations to the end)
    assert len(subprocess.check_output([out, "args"], text=True, env=env).splitlines()) == 28
    solid = noise_world(5, (16, 128, 16), 0.4)
    seeds = seeds_of(np.random.default_rng(2), solid.shape, 9, 4)
    queries = [((-1, 50, -1), (17, 131, 17), seeds, medium, 0x3F, 70, order) for medium in (AIR, SOLID) for order in (False, True)]
    ws = world_of(solid)
    try:
        results = run_fields(out, tmp_path, ws, queries, env=env)
    finally:
        ws.close()
    for (lo, hi, seeds, medium, mask, cut, _), (got, totals) in zip(queries, results):
        want, summary = spreadmodel.field(solid, lo, hi, seeds, medium, mask, cut)
        assert (got == want).all() and same_totals(totals, summary)


# ---- the argument check -----------------------------------------------------------------------------------------------------------------------------

def test_every_rejection_has_its_message_and_the_boundary_values_pass(rules):
    lines = [line.split("|", 1) for line in subprocess.check_output([rules, "args"], text=True).splitlines()]
    got = [(int(code), message) for code, message in lines]
    want = [
        (-1, ""), (-1, ""),
        (-1, "cvx_world_spread: params is NULL"), (-1, "cvx_world_spread: seeds is NULL"), (-1, "cvx_world_spread: out is NULL"),
        (-1, "cvx_world_spread_device: out is NULL"),
        (-1, "cvx_world_spread: the box [0, 0) on axis 1 is empty"),
        (-1, "cvx_world_spread: the box [-1073741825, 2) on axis 0 has a coordinate beyond 2^30"),
        (-1, "cvx_world_spread_device: the box [0, 1073741825) on axis 2 has a coordinate beyond 2^30"),
        (-1, "cvx_world_spread: a box of 2^31 or more voxels"),
        (-1, "cvx_world_spread: bad medium 2"), (-1, "cvx_world_spread_device: bad medium -1"),
        (-1, "cvx_world_spread: stepFaces is zero"), (-1, "cvx_world_spread: stepFaces 0x40 has bits above 0x3F"),
        (-1, "cvx_world_spread: maxSteps 0 outside 1 .. 65534"), (-1, "cvx_world_spread_device: maxSteps 65535 outside 1 .. 65534"),
        (-1, "cvx_world_spread: seedCount 0 outside 1 .. 4096"), (-1, "cvx_world_spread: seedCount 4097 outside 1 .. 4096"),
        (-1, "cvx_world_spread: seed 5: start 11 outside 0 .. maxSteps 10"), (-1, "cvx_world_spread_device: seed 5: start -1 outside 0 .. maxSteps 10"),
        (-1, "cvx_world_spread: bad medium 7"), (-1, "cvx_world_spread: the box [0, 0) on axis 0 is empty"),
    ] + [(-3, "world LOD 0 has not been uploaded")] * 6  # valid arguments on a context without a world: CVX_ERR_NOT_READY
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w] or (len(got), len(want))


def test_python_wrappers_check_their_arguments():
    ctx = object.__new__(gpu.Context)
    with pytest.raises(ValueError, match="three integers"):
        gpu.Context.world_spread(ctx, (0, 0), (1, 1, 1), [(0, 0, 0)], medium=AIR, max_steps=4)
    with pytest.raises(ValueError, match="a seed is"):
        gpu.Context.world_spread(ctx, (0, 0, 0), (1, 1, 1), [(0, 0)], medium=AIR, max_steps=4)
    with pytest.raises(ValueError, match="int32 device tensor"):
        gpu.Context.world_spread_device(ctx, (0, 0, 0), (1, 1, 1), [(0, 0, 0)], np.zeros(1, dtype=np.int32), medium=AIR, max_steps=4)
    s = gpu.seeds_array([(1, 2, 3), (4, 5, 6, 7)])
    assert s.dtype == gpu.SPREAD_SEED_DTYPE and s["voxel"].tolist() == [[1, 2, 3], [4, 5, 6]] and s["start"].tolist() == [0, 7]
    assert gpu.seeds_array(s) is s or (gpu.seeds_array(s) == s).all()


# ---- wrappers and documents -------------------------------------------------------------------------------------------------------------------------------------------

def test_the_documents_name_the_call():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"all {len(gpu.EXPORTS)} exports" in readme and "all 64 exports" in readme
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("tools", "README.md"), os.path.join("profiles", "spread.md")):
        assert "spread" in open(os.path.join(ROOT, name)).read(), name
