"""CPU (no GPU needed): the worlds and cases of tests/test_gpu_world_oblong.py on the dense models alone, and the host-compiled rules on both sizes.

- The worlds can tell the axes apart: a column and the column a row length taken from dimX would find instead differ in at least 90 % of the
  pairs, and so do (x, z) and (z, x) in the square corner.  90 % is a floor that keeps a world from hiding a swap, not a tolerance.
- Every case of the GPU file reaches past the short side: its writers change columns beyond it and the far corner column; its readers' expected
  results hold something beyond it; per-face flags set the X bits differently from the Z bits and the model's result depends on that.
- Every rule program with a mode that takes a world blob and its dims, on both sizes against the dense models, with the calls of the GPU cases:
  move `world` (bounded and repeating), snapshot `world`, spread `fields`, distance `fields`, readback `level` (all six levels, both worlds), light,
  pieces, settle, cavity, copy, dense, models and lamp `world`, surface and surface_rects `world`, nav `world`, dense, heights and models `read`,
  brush `pick`.  snapshot and spread run as the -fsanitize=address,undefined stand-alone builds their own test files make.  Left out, because they
  have no such mode: stamp_rules and shape_rules (triangles and strokes in, spans out; no world), device_call_rules (no world), and the `columns` /
  `cases` / `shade` / `args` modes of the others, which take single columns or no world at all."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import copymodel
import densemodel
import distancemodel
import heightsmodel
import lampmodel
import modelsmodel
import lightmodel
import oblongworlds as ob
import pickmodel
import piecesmodel
import ruleslib
import settlemodel
import scenes
import snapshotmodel
import spreadmodel
from cpuvox_amd import gpu
from oblongworlds import LONG_X, LONG_Z, SIZES
from test_gpu_world_brush import _brushed
from test_world_brush_cpu import _run_pick
from test_world_cavities_cpu import _check_calls as check_cavities
from test_world_copy_cpu import _run_world as copy_world
from test_world_copy_cpu import rectangle as copy_rectangle
from test_world_dense_cpu import _run_world as dense_world
from test_world_distance_cpu import _run_fields as distance_fields
from test_world_heights_cpu import write_box
from test_world_light_cpu import model_world
from test_world_light_cpu import run_world as light_world
from test_world_nav_cpu import assert_field as assert_nav_field
from test_world_nav_cpu import run_world as nav_world
from test_world_models_cpu import _check_call as check_models
from test_world_models_cpu import _run_read as models_read
from test_world_move_cpu import bodies_to_array, model_results, world_bodies
from test_world_move_cpu import run_world as move_world
from test_world_pieces_cpu import GROUND, pieces_rows
from test_world_pieces_cpu import run_world as pieces_world
from test_world_settle_cpu import run_world as settle_world
from test_world_settle_cpu import settle_rectangle
from test_world_sequences_later_cpu import headroom, read_map, slots_in_use, work  # noqa: F401  (work: the fixture)
from test_world_snapshot_cpu import IGNORE, as_xzy
from test_world_snapshot_cpu import run_world as snapshot_world
from test_world_spread_cpu import run_fields, same_totals
from test_world_surface_cpu import _check_calls as check_surface
from test_world_surface_rects_cpu import check_call as check_surface_rects

SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (the HIP runtime the library links keeps its own allocations to the end)
WRITER_NAMES = sorted(ob.writer_cases(LONG_Z))
READER_NAMES = sorted(ob.reader_cases(LONG_Z))


SANITIZED = ("snapshot_rules", "spread_rules")  # (the test files of these two build them so themselves)


class _Programs:
    """tests/<name>_rules.cpp compiled on first use, each a stand-alone program (its own main; nothing is loaded into Python): programs["move"]."""

    def __init__(self, directory):
        self.directory, self.built = directory, {}

    def __getitem__(self, name):
        if name not in self.built:
            self.built[name] = ruleslib.build(name + "_rules", self.directory, *(SANITIZE if name + "_rules" in SANITIZED else ()))
        return self.built[name]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    return _Programs(tmp_path_factory.mktemp("oblong"))


def _far(dims):
    return dims[0] - 1, dims[2] - 1


# ---- the sizes and the worlds -------------------------------------------------------------------------------------------------------------------------

def test_the_sizes_separate_the_axes():
    for dims, row_shift in ((LONG_Z, 8), (LONG_X, 5)):
        assert dims[0] * dims[2] == 8192 and dims[2] == 1 << row_shift
        assert all(d >> 5 >= 1 for d in dims), "all six LODs"
        assert ob.short_side(dims) == 32, "one levelCount-5 rounding unit"
    assert ob.swap_xz(ob.X_AND_Z) == 0x10 | 0x02 and ob.swap_xz(0x3F) == 0x3F and ob.swap_xz(0x04) == 0x04


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("sparse", [False, True])
def test_the_worlds_can_tell_the_axes_apart(programs, tmp_path, dims, sparse):
    solid, colour = ob.volumes(dims, sparse)
    aliased, transposed = ob.distinct_fractions(solid, colour)
    print(f"{dims} sparse {sparse}: {aliased:.4f} of the aliased pairs and {transposed:.4f} of the transposed pairs differ")
    assert aliased >= 0.9 and transposed >= 0.9, (aliased, transposed)
    if not sparse:
        assert aliased == 1.0 and transposed == 1.0, "the dense world at seed 61 separates every pair"
    columns = solid.any(axis=1)
    assert ob.beyond(dims, columns) and columns[_far(dims)], "read_region, read_level and download return columns past the short side"
    # the layout, as the sparse tests of the world calls establish it: what cvx_world_upload chose for LOD 0
    _, _, ws = (ob.sparse_world if sparse else ob.dense_world)(dims)
    try:
        bodies = bodies_to_array(world_bodies(ob.SEED, solid, False, 4))
        _, colour_shift, listed, _ = move_world(programs["move"], tmp_path, ws.storage(0).tobytes(), dims, ws.info(0).columnCount, False, bodies)
    finally:
        ws.close()
    assert colour_shift == (2 if sparse else 7) and (sparse or listed > 0)


# ---- every case reaches past the short side -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("name", WRITER_NAMES)
def test_a_writing_case_reaches_past_the_short_side(work, dims, name):
    written = np.zeros((dims[0], dims[2]), dtype=bool)
    levels = set()
    for plan in ob.writer_cases(dims)[name]:
        m = ob.OblongModels(dims, *ob.volumes(dims), work)
        m.run(plan)
        partial = [k for k, (_, args) in enumerate(plan) if args.get("level_count", 5) < 5]
        assert partial in ([], [len(plan) - 1]), "a step below levelCount 5 ends its run"
        levels |= {args.get("level_count", 5) for _, args in plan}
        if plan[-1][0] in ob.WRITERS:
            assert ob.beyond(dims, m.last), f"{plan[-1][1]['label']} changes nothing past the short side"
            written |= m.last
    assert ob.beyond(dims, written) and written[_far(dims)], f"{name} does not change the far corner column"
    if name not in ("set_columns", "rounds to the short side"):
        assert levels >= {0, 2, 5}, levels


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("name", READER_NAMES)
def test_a_reading_case_reaches_past_the_short_side(work, dims, name):
    m = ob.OblongModels(dims, *ob.volumes(dims), work)
    for step in ob.reader_cases(dims)[name]:
        m.seen[:] = False
        m.run([step])
        if step[0] not in ob.WRITERS:
            assert ob.beyond(dims, m.seen), f"{step[1]['label']}: nothing past the short side"
    assert name in ob.NEEDS_SHELLS or not m.written.any()


@pytest.mark.parametrize("dims", SIZES)
def test_the_other_cases_reach_past_the_short_side(dims):
    """The cases of the GPU file that are no call lists: the rounding case, the rejected copy, the moves, the picks and the relayout's terrain (the
    forty strokes of the snapshot's diff and the compaction: test_the_towers_reach_past_the_short_side, on both worlds)."""
    solid, colour = ob.volumes(dims)
    dx, dy, dz = dims
    assert ob.rounded((dx - 3, dz - 3, 3, 3), 5, dims) == (dx - 32, dz - 32, 32, 32) and 32 in (dx, dz), "the rectangle rounds to exactly the short side"
    # copy: the source is legal only where its 40 columns are measured against the long side
    lo, hi = ob.copy_source(dims)
    assert all(hi[a] <= dims[a] for a in range(3)) and not all(hi[a] <= dims[2 - a] for a in range(3))
    bad = ob.copy_rejected(dims)
    assert any(bad["srcMax"][a] > dims[a] for a in (0, 2)) and all(bad["srcMax"][a] <= dims[2 - a] for a in (0, 2)), "it would fit if the axes were swapped"
    # moves: random bodies end past the short side, resting and blocked; the seam bodies are blocked or come to rest on the far side of a seam
    U = gpu.MOVE_UNIT
    for repeat in (False, True):
        bodies = world_bodies(ob.SEED, solid, repeat, 600) + ob.seam_bodies(dims)
        want = model_results(solid, bodies, repeat)
        cols = np.zeros((dx, dz), dtype=bool)
        touched = (want["flags"] & 0x7F) != 0
        x, z = want["pos"][touched][:, 0] // U, want["pos"][touched][:, 2] // U
        inside = (x >= 0) & (x < dx) & (z >= 0) & (z < dz)
        cols[x[inside], z[inside]] = True
        assert ob.beyond(dims, cols) and touched.sum() > 100, repeat
        seam = want[-len(ob.seam_bodies(dims)):]
        if repeat:
            first = np.array([b["pos"] for b in ob.seam_bodies(dims)])
            crossed = (seam["pos"][:, 0] // (dx * U) != first[:, 0] // (dx * U)) | (seam["pos"][:, 2] // (dz * U) != first[:, 2] // (dz * U))
            assert crossed.sum() >= len(seam) // 2, "the seam bodies cross the seams"
            assert (np.array(seam["pos"][:, 0] // (dx * U)) != first[:, 0] // (dx * U)).any() and (seam["pos"][:, 2] // (dz * U) != first[:, 2] // (dz * U)).any()
    # picks: bounded rays hit past the short side; repeating rays leave through each side and hit behind the seam
    o, d, max_t = pickmodel.random_rays(np.random.default_rng(5), dims, 600)
    vox, face, _, _, _ = pickmodel.pick_many(solid, colour, o, d, max_t)
    cols = np.zeros((dx, dz), dtype=bool)
    cols[vox[face >= 0][:, 0], vox[face >= 0][:, 2]] = True
    assert ob.beyond(dims, cols)
    o, d, side = ob.seam_rays(dims, 200)
    t_solid, t_colour, at = ob.tiled(dims, solid, colour)
    vox, face, _, _, _ = pickmodel.pick_many(t_solid, t_colour, o + at, d, ob.SEAM_MAX_T)
    for s in range(4):
        hit = (face >= 0) & (side == s)
        tile = vox[hit][:, [0, 2]] // np.array([dx, dz]) - (at[[0, 2]] // np.array([dx, dz])).astype(np.int64)
        assert (tile != 0).any(axis=1).sum() >= 3, f"rays through side {s} re-enter and hit"
    write = ob.relayout_write(dims)
    assert write[2].shape == (dx, dz) and write[2].min() >= 44


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("sparse", [False, True])
def test_the_towers_reach_past_the_short_side(dims, sparse):
    """The forty strokes of the snapshot's diff and of the compaction, on both worlds: they change columns along the whole long axis, and the diff
    of the whole footprint extends to its far end."""
    solid, colour = ob.volumes(dims, sparse)
    dx, _, dz = dims
    after = _brushed(solid, colour, ob.tower_strokes(dims, 40))
    changed = ((after[0] != solid) | (after[1] != colour)).any(axis=1)
    assert ob.beyond(dims, changed) and changed[:, : dz // 2].any() and changed[: dx // 2].any(), "the towers stand along the whole long axis"
    changes, summary = snapshotmodel.diff(as_xzy(solid, colour), as_xzy(*after))
    cols = np.zeros((dx, dz), dtype=bool)
    cols[changes["x"], changes["z"]] = True
    assert ob.beyond(dims, cols) and (summary["max"][0] > dx - 16 if dx > dz else summary["max"][2] > dz - 16), summary
    for box in (ob.corner(dims), ob.overhang(dims)):  # the other snapshots of the diff case
        x0, z0, sx, sz = ob.rounded(ob.rect_of(box), 0, dims)
        assert ob.beyond(dims, cols & (np.arange(dx)[:, None] >= x0) & (np.arange(dz)[None, :] >= z0)), box


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("sparse", [False, True])
def test_the_terrain_does_not_fit_the_tails(dims, sparse):
    """From the volumes alone: the colour slots that must move to LOD 0's tail when the terrain is written exceed the most that tail can hold
    behind a compaction (an eighth of an upper bound of the slots in use, 16384 at the least).  Colour blocks: a column's block lies within 7
    columns of it and is as deep as its deepest column, so a column that gets more voxels than any column within 7 of it had moves with its
    block.  Column after column: a column that gets more voxels than it had moves."""
    solid, colour = ob.volumes(dims, sparse)
    old = _brushed(solid, colour, ob.tower_strokes(dims, 40))[0]
    heights = ob.relayout_write(dims)[2]
    counts_old, counts_new = old.sum(axis=1), heights
    room = counts_old if sparse else ndimage.maximum_filter(counts_old, size=15, mode="constant")
    need = int(counts_new[counts_new > room].sum())
    assert need > 2 * headroom(slots_in_use(old)), (need, headroom(slots_in_use(old)))


@pytest.mark.parametrize("name", ["stripes32x64x128", "proc128x64x32"])
def test_the_repeat_render_worlds_are_oblong(name):
    ws = scenes.load_world(name)
    assert ws.dims[0] != ws.dims[2] and min(ws.dims[0], ws.dims[2]) >= 32, ws.dims


# ---- the rule programs that take a world blob and its dims ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("repeat", [False, True])
def test_move_rules_world(programs, tmp_path, dims, repeat):
    solid, _, ws = ob.dense_world(dims)
    try:
        bodies = world_bodies(ob.SEED, solid, repeat, 1000) + ob.seam_bodies(dims)
        got, colour_shift, listed, _ = move_world(programs["move"], tmp_path, ws.storage(0).tobytes(), dims, ws.info(0).columnCount, repeat, bodies_to_array(bodies))
    finally:
        ws.close()
    want = model_results(solid, bodies, repeat)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"repeat {repeat}: {len(bad)} bodies differ; first {bodies[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"
    assert colour_shift == 7 and listed > 0


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("sparse", [False, True])
def test_snapshot_rules_world(programs, tmp_path, dims, sparse):
    """The arena holds the world after the towers, the snapshot is the world before them: three rectangles, both flags."""
    solid, colour, before = (ob.sparse_world if sparse else ob.dense_world)(dims)
    after_dense = _brushed(solid, colour, ob.tower_strokes(dims, 40))
    after = model_world(dims, *after_dense)
    try:
        for rect in (ob.rect_of(ob.whole(dims)), ob.rect_of(ob.corner(dims)), (dims[0] - 32, dims[2] - 32, 32, 32)):
            x0, z0, sx, sz = rect
            cut = lambda v: tuple(a[x0:x0 + sx, z0:z0 + sz] for a in as_xzy(*v))  # noqa: E731
            for flags in (0, IGNORE):
                want, want_summary = snapshotmodel.diff(cut((solid, colour)), cut(after_dense), (x0, z0), flags)
                got, summary = snapshot_world(programs["snapshot"], tmp_path, after, dims, before.extract_region(0, *rect)[0], rect, flags, SAN_ENV)
                assert summary == want_summary and got.tobytes() == want.tobytes(), (rect, flags, summary, want_summary)
                assert len(want) > 0
    finally:
        before.close()
        after.close()


@pytest.mark.parametrize("dims", SIZES)
def test_spread_rules_fields(programs, tmp_path, dims):
    solid, _, ws = ob.dense_world(dims)
    steps = ob.reader_cases(dims)["spread"]
    queries = [(*a["box"], a["seeds"], a["medium"], a.get("step_faces", 0x3F), a["max_steps"], order) for _, a in steps for order in (False, True)]
    try:
        results = run_fields(programs["spread"], tmp_path, ws, queries, env=SAN_ENV)
    finally:
        ws.close()
    for (lo, hi, seeds, medium, mask, cut, order), (got, totals) in zip(queries, results):
        want, summary = spreadmodel.field(solid, lo, hi, seeds, medium, mask, cut)
        bad = got != want
        assert not bad.any(), f"medium {medium} mask {mask:#x} box {lo} .. {hi} reversed {order}: {int(bad.sum())} of {bad.size} differ"
        assert same_totals(totals, summary), (totals, summary)


@pytest.mark.parametrize("dims", SIZES)
def test_light_rules_world(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        for plan in ob.writer_cases(dims)["light"]:
            for _, args in plan[:1]:
                p, level_count = args["p"], args.get("level_count", 5)
                rect, got, colour_shift, listed, over, voxels, _ = light_world(programs["light"], tmp_path, ws, p, level_count)
                assert colour_shift == 7 and listed > 0 and over == 0
                assert rect == lightmodel.rectangle(p, dims, level_count), args["label"]
                want_ws = model_world(dims, solid, lightmodel.light(solid, colour, p))
                try:
                    assert got == want_ws.extract_region(0, *rect)[0], f"{args['label']}: the sub-world blob of {rect} differs from the model's"
                finally:
                    want_ws.close()
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_pieces_rules_world(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        for box, level_count in ((ob.corner(dims), 0), (ob.corner(dims), 2), (ob.overhang(dims), 5)):
            want_pieces, want_summary, _ = piecesmodel.analyse(solid, *box, GROUND)
            summary, pieces, rect, got, colour_shift, listed, over, _, _ = pieces_world(programs["pieces"], tmp_path, ws, *box, GROUND, level_count)
            assert colour_shift == 7 and listed > 0 and over == 0
            assert summary == want_summary and pieces_rows(pieces) == pieces_rows(want_pieces), box
            assert rect == piecesmodel.rectangle(want_pieces, dims, level_count), box
            want_ws = model_world(dims, *piecesmodel.remove(solid, colour, *box, GROUND))
            try:
                assert got == want_ws.extract_region(0, *rect)[0], f"{box}: the sub-world blob of {rect} differs from the model's"
            finally:
                want_ws.close()
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_pick_rules_world(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        o, d, max_t = pickmodel.random_rays(np.random.default_rng(5), dims, 2000)
        hits, colour_shift, listed = _run_pick(programs["brush"], tmp_path, ws, o, d, max_t)
    finally:
        ws.close()
    assert colour_shift == 7 and listed > 0
    fraction = pickmodel.compare_picks(hits, pickmodel.pick_many(solid, colour, o, d, max_t), f"{dims}")
    assert fraction >= 0.99, f"only {fraction:.4f} of the rays are unambiguous"


def _steps(cases, call):
    """The arguments of every step `call` in a dict of cases (writer cases: lists of runs; reader cases: one run)."""
    runs = [run for case in cases.values() for run in (case if isinstance(case[0], list) else [case])]
    return [args for run in runs for c, args in run if c == call]


@pytest.mark.parametrize("dims", SIZES)
def test_distance_rules_fields(programs, tmp_path, dims):
    solid, _, ws = ob.dense_world(dims)
    queries = [(*a["box"], a.get("R", 8), a["mode"], a["solid_outside"]) for a in _steps(ob.reader_cases(dims), "distance")]
    assert len(queries) == 9
    try:
        fields = distance_fields(programs["distance"], tmp_path, ws, queries)
    finally:
        ws.close()
    for (lo, hi, R, mode, outside), got in zip(queries, fields):
        want = distancemodel.field(solid, (lo, hi), R, mode, outside)
        bad = got != want
        assert not bad.any(), f"mode {mode} solidOutside {outside:#x} box {lo} .. {hi}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("sparse", [False, True])
def test_readback_rules_level(programs, tmp_path, dims, sparse):
    """Every level uploaded into a host-only context and read back: the host twin of the read-back's and the compaction's usedX / usedZ / blocksZ."""
    _, _, ws = (ob.sparse_world if sparse else ob.dense_world)(dims)
    shifts = []
    try:
        for lod in range(6):
            blob = ws.storage(lod).tobytes()
            (tmp_path / "blob").write_bytes(blob)
            out = subprocess.check_output([programs["readback"], "level", str(tmp_path / "blob"), str(lod), *[str(d) for d in dims], str(ws.info(lod).columnCount),
                                           str(tmp_path / "out")], text=True)
            shifts.append(out.split()[1])
            assert (tmp_path / "out").read_bytes() == blob, f"LOD {lod}"
    finally:
        ws.close()
    assert shifts[0] == ("2" if sparse else "7"), shifts


@pytest.mark.parametrize("dims", SIZES)
def test_settle_rules_world(programs, tmp_path, dims):
    """The settle steps of the writing cases, each on the world its run gives it (the floating block over the far corner)."""
    for run in ob.writer_cases(dims)["settle"]:
        m = ob.OblongModels(dims, *ob.volumes(dims), None)
        m.run(run[:-1])
        a = run[-1][1]
        level_count, max_drop = a.get("level_count", 5), a.get("max_drop", 0)
        colour = np.where(m.solid, m.colour, 0).astype(m.colour.dtype)
        want_pieces, want_drops, want_summary, (s, c) = settlemodel.settle(m.solid, colour, *a["box"], a["anchors"], max_drop)
        ws = model_world(dims, m.solid, colour)
        try:
            summary, pieces, drops, rect, got, over, _, _, _ = settle_world(programs["settle"], tmp_path, ws, *a["box"], a["anchors"], max_drop, level_count)
        finally:
            ws.close()
            (tmp_path / "world.bin").unlink()  # (the driver keeps a blob it finds)
        assert over == 0 and summary == want_summary and pieces_rows(pieces) == pieces_rows(want_pieces) and drops.tolist() == want_drops.tolist(), a["label"]
        assert rect == settle_rectangle(want_pieces, want_drops, dims, level_count), a["label"]
        x0, z0, sx, sz = rect
        got_solid, got_colour = piecesmodel.decode_blob(got, (sx, dims[1], sz))
        assert (got_solid == s[x0:x0 + sx, :, z0:z0 + sz]).all() and (got_colour == c[x0:x0 + sx, :, z0:z0 + sz]).all(), a["label"]


@pytest.mark.parametrize("dims", SIZES)
def test_cavity_rules_world(programs, tmp_path, dims):
    """The FILL steps of the writing cases and the REPORT boxes of the reading case, on the world with the four shells."""
    m = ob.OblongModels(dims, *ob.volumes(dims), None)
    m.run(ob.shell_steps(dims))
    ws = model_world(dims, m.solid, m.colour)
    try:
        for level_count in (0, 2, 5):
            calls = {a["label"]: (*a["box"], a.get("open_faces", 0x3F), a.get("max_voxels", 0))
                     for a in _steps(ob.writer_cases(dims), "fill_cavities") + _steps(ob.reader_cases(dims), "report_cavities") if a.get("level_count", 5) == level_count}
            assert check_cavities(programs["cavity"], tmp_path, m.solid, m.colour, ws, dims, calls, level_count) == len(calls) >= 1
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_surface_and_surface_rects_rules_world(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        calls = {a["label"]: (*a["box"], a["solid_outside"], a.get("flags", 0)) for a in _steps(ob.reader_cases(dims), "surface")}
        assert len(calls) == 3
        check_surface(programs["surface"], tmp_path, solid, colour, ws, calls)
        for a in _steps(ob.reader_cases(dims), "surface_rects"):
            check_surface_rects(programs["surface_rects"], tmp_path, solid, colour, ws, *a["box"], a["solid_outside"], a.get("flags", 0), a["label"])
            (tmp_path / "world.bin").unlink(missing_ok=True)
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_nav_rules_world(programs, tmp_path, dims):
    solid, _, ws = ob.dense_world(dims)
    try:
        for a in _steps(ob.reader_cases(dims), "nav"):
            steps, summary, _, _ = nav_world(programs["nav"], tmp_path, ws, *a["call"], a["goals"])
            assert assert_nav_field(steps, summary, solid, a["call"], a["goals"], a["label"])["reached"] > 0
    finally:
        ws.close()


def _region(dims, solid, colour, rect):
    ws = model_world(dims, solid, colour)
    try:
        return ws.extract_region(0, *rect)[0]
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_copy_rules_world(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        steps = _steps(ob.writer_cases(dims), "copy")
        assert len(steps) == 4 and any(p["transform"] & 1 for a in steps for p in a["placements"])
        for a in steps:
            rect = copy_rectangle(a["placements"], dims, a.get("level_count", 5))
            s, c = copymodel.apply_copies(solid, colour, gpu.copy_placements_array(a["placements"]))
            got, colour_shift, listed, over = copy_world(programs["copy"], tmp_path, ws, a["placements"], rect)
            assert over == 0 and colour_shift == 7 and listed > 0
            assert got == _region(dims, s, c, rect), f"{a['label']}: the sub-world blob of {rect} differs from the model's"
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_dense_rules_world_and_read(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        steps = _steps({"write_voxels": ob.writer_cases(dims)["write_voxels"]}, "write_voxels")
        assert len(steps) == 4
        for a in steps:
            at, argb, mask, op = a["write"]
            shape = (argb if argb is not None else mask).shape
            box = (tuple(at), (at[0] + shape[0], at[1] + shape[2], at[2] + shape[1]))
            rect = densemodel.rectangle(box, dims, a.get("level_count", 5))
            s, c = densemodel.write(solid, colour, box, argb, mask, op)
            got, colour_shift, listed, over = dense_world(programs["dense"], tmp_path, ws, (at, argb, mask, op), rect)
            assert over == 0 and colour_shift == 7 and listed > 0
            assert got == _region(dims, s, c, rect), f"{a['label']}: the sub-world blob of {rect} differs from the model's"
        info = ws.info(0)
        for a in _steps(ob.reader_cases(dims), "read_voxels"):
            lo, hi = a["box"]
            size = [hi[i] - lo[i] for i in range(3)]
            subprocess.check_call([programs["dense"], "read", str(tmp_path / "world.bin"), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                   *[str(v) for v in lo], *[str(v) for v in size], str(tmp_path / "read.bin")])
            raw = (tmp_path / "read.bin").read_bytes()
            n, shape = size[0] * size[1] * size[2], (size[0], size[2], size[1])
            want_argb, want_mask = densemodel.read(solid, colour, (lo, hi))
            assert (np.frombuffer(raw[:4 * n], dtype=np.uint32).reshape(shape) == want_argb).all(), a["label"]
            assert (np.frombuffer(raw[4 * n:], dtype=np.uint8).reshape(shape) == want_mask).all(), a["label"]
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_models_rules_world_and_read(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        steps = _steps(ob.writer_cases(dims), "place_models")
        assert len(steps) == 3
        for a in steps:
            check_models(programs["models"], tmp_path, (dims, solid, colour, ws), a["models"], a["instances"], a.get("level_count", 5), a["label"])
        for a in _steps(ob.reader_cases(dims), "read_model"):
            dst_size, instance = read_map(dims, a["src_min"], a["size"], a["transform"])
            d = modelsmodel.from_struct(instance)
            argb, mask = models_read(programs["models"], tmp_path, ws, dst_size, d["m"], d["t"])
            want = modelsmodel.read(solid, colour, dst_size, d["m"], d["t"])
            assert (argb == want[0]).all() and (mask == want[1]).all(), a["label"]
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_heights_rules_read(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        info = ws.info(0)
        (tmp_path / "world.bin").write_bytes(ws.storage(0).tobytes())
        boxes = [(a["label"], a["box"]) for a in _steps(ob.reader_cases(dims), "read_heights")]
        boxes += [(a["label"], write_box(a["write"])) for a in _steps(ob.writer_cases(dims), "write_heights")]  # (the windows of the writes, read)
        for label, (lo, hi) in boxes:
            size = [hi[i] - lo[i] for i in range(3)]
            subprocess.check_call([programs["heights"], "read", str(tmp_path / "world.bin"), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                   *[str(v) for v in lo], *[str(v) for v in size], str(tmp_path / "read.bin")])
            n = size[0] * size[2]
            raw = np.frombuffer((tmp_path / "read.bin").read_bytes(), dtype=np.uint32)
            assert raw.size == 3 * n
            got = raw[:n].view(np.int32).reshape(size[0], size[2]), raw[n:2 * n].reshape(size[0], size[2]), raw[2 * n:].view(np.int32).reshape(size[0], size[2])
            for g, w, what in zip(got, heightsmodel.read(solid, colour, (lo, hi)), ("heights", "argb", "bottoms")):
                assert (g == w).all(), f"{label}: {what}"
    finally:
        ws.close()


@pytest.mark.parametrize("dims", SIZES)
def test_lamp_rules_world(programs, tmp_path, dims):
    solid, colour, ws = ob.dense_world(dims)
    try:
        info = ws.info(0)
        (tmp_path / "world.bin").write_bytes(ws.storage(0).tobytes())
        steps = _steps(ob.writer_cases(dims), "lamps")
        assert len(steps) == 3
        for a in steps:
            p, lamps, level_count = a["p"], a["lamps"], a.get("level_count", 5)
            (tmp_path / "lamps.bin").write_bytes(np.array(lampmodel.words(lamps)[1:], dtype=np.int32).tobytes())
            text = subprocess.check_output([programs["lamp"], "world", str(tmp_path / "world.bin"), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                            *[str(v) for v in lightmodel.words(p)], str(level_count), str(tmp_path / "lamps.bin"), str(tmp_path / "sub.bin")], text=True)
            m = re.match(r"rect (\d+) (\d+) (\d+) (\d+) voxels (\d+)", text)
            assert m, text
            rect = tuple(int(m.group(k)) for k in range(1, 5))
            assert rect == lightmodel.rectangle(p, dims, level_count), a["label"]
            want = _region(dims, solid, lampmodel.light(solid, colour, p, lamps), rect)
            assert (tmp_path / "sub.bin").read_bytes() == want, f"{a['label']}: the sub-world blob of {rect} differs from the model's"
    finally:
        ws.close()
