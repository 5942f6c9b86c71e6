"""GPU: snapshots of rectangles of the device-resident world (include/cpuvox_gpu_snapshot.h): cvx_world_snapshot, cvx_world_snapshot_restore,
cvx_world_snapshot_diff / _device.

Everything is bytes and integers: a restore is checked by cvx_world_read_region / cvx_world_read_level giving, byte for byte, what they gave
when the snapshot was taken; a diff against the dense model of tests/snapshotmodel.py on what cvx_world_read_voxels gives before and after.
The worlds are the small ones of the sequence tests (DIMS = 128 x 64 x 128, dense and sparse), the 32 x 256 x 32 tall world and the terrain of
the edit tests."""
import numpy as np
import pytest
import torch

import lightmodel
import oraclelib as O
import scenes
import snapshotmodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _box, _brushed, _dense, _sphere
from test_gpu_world_dense import TALL, _any_world, _tall_solid
from test_gpu_world_edit import BOTH_KERNELS, CLEAR, H, W, _assert_same, _frames, _terrain, _world
from test_gpu_world_sequences import DIMS, STROKES
from test_world_brush_cpu import _pick_world
from test_world_light_cpu import RGB, model_world
from test_world_pieces_cpu import GROUND
from test_world_sequences_later_cpu import assert_foreign, group_box, group_columns, group_plan

pytestmark = pytest.mark.gpu

FILL, CARVE, PAINT, REPLACE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT, gpu.COPY_REPLACE
IGNORE = gpu.SNAPSHOT_IGNORE_COLOUR
WHOLE = (0, 0, DIMS[0], DIMS[2])
ODD = (50, 55, 21, 23)   # 483 columns at levelCount 0, 24 x 28 = 672 at 2: no multiple of 64 (at 5 every rectangle of this world is one of 1024)
ONE = (24, 24, 1, 1)     # under a floating slab
SUN = dict(sun_dir=(3, 4, 1), sun_level=150, sun_range=64, sky_level=80, sky_range=6, floor_level=25)


def _context(ws):
    ctx = gpu.Context(0)
    ctx.upload_world(ws)
    return ctx


@pytest.fixture(scope="module")
def dense_world():
    solid, colour, ws = _pick_world(np.random.default_rng(61), DIMS)
    yield solid, colour, ws
    ws.close()


def levels(ctx):
    """Every level whole, as it reads back."""
    return [ctx.read_level(k) for k in range(6)]


def regions(ctx, rect, level_count):
    return [ctx.read_region(k, *[v >> k for v in rect]) for k in range(level_count + 1)]


def held(snapshot):
    i = snapshot.info
    return i["x0"], i["z0"], i["sizeX"], i["sizeZ"]


def rounded(rect, level_count, dims=DIMS):
    a = (1 << level_count) - 1
    x0, z0 = rect[0] & ~a, rect[1] & ~a
    x1, z1 = min((rect[0] + rect[2] + a) & ~a, dims[0]), min((rect[1] + rect[3] + a) & ~a, dims[2])
    return x0, z0, x1 - x0, z1 - z0


def assert_levels(got, want, label):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{label}: LOD {k} differs"


def voxels(ctx, dims=DIMS):
    """(solid, argb) of the whole world as (X, Z, Y) arrays: what the model compares."""
    argb, solid = ctx.read_voxels((0, 0, 0), dims)
    return solid, argb


def cut(volume, rect):
    x0, z0, sx, sz = rect
    return tuple(a[x0:x0 + sx, z0:z0 + sz] for a in volume)


# ---- 1. the round trip --------------------------------------------------------------------------------------------------------------------------------

def writers(rect, level_count):
    """The writers of the issue, each over the rectangle's own columns: (name, call)."""
    x0, z0, sx, sz = rect
    lo, hi = (x0, 0, z0), (x0 + sx, DIMS[1], z0 + sz)
    dense = np.random.default_rng(5).integers(1, 2**32, size=(sx, sz, 30), dtype=np.uint64).astype(np.uint32)
    dense[::2, :, ::3] = 0
    return [
        ("brush FILL", lambda c: c.brush([_box(FILL, (x0, 20, z0), (x0 + sx, 40, z0 + sz), 0xFF2040F0)], level_count)),
        ("brush CARVE", lambda c: c.brush([_box(CARVE, (x0, 0, z0), (x0 + sx, 12, z0 + sz))], level_count)),
        ("brush PAINT", lambda c: c.brush([_box(PAINT, lo, hi, 0xFF00C0FF)], level_count)),
        ("light to RGB", lambda c: c.world_light(lo, hi, target=RGB, level_count=level_count, **SUN)),
        ("settle", lambda c: c.world_settle(lo, hi, GROUND, 0, level_count, 64)),
        ("write_voxels", lambda c: c.write_voxels((x0, 5, z0), dense, None, REPLACE, level_count)),
    ]


@pytest.mark.parametrize("rect, level_count", [(ONE, 0), (ODD, 0), (ODD, 2), (ODD, 5), (WHOLE, 0), (WHOLE, 2), (WHOLE, 5)])
def test_restore_takes_every_writer_back(dense_world, rect, level_count):
    """Snapshot, write, restore: cvx_world_read_region of every held level gives the bytes taken before, and so does every whole level -- the
    columns around the rectangle and the levels above levelCount included.  One snapshot serves all six writers: it is restored six times."""
    ctx = _context(dense_world[2])
    try:
        ctx.brush([STROKES[0]], 5)  # (the levels have an edit tail and a moved colour block before the first snapshot)
        before = levels(ctx)
        with ctx.world_snapshot(*rect, level_count) as snapshot:
            got = held(snapshot)
            assert got == rounded(rect, level_count) and snapshot.info["levelCount"] == level_count
            assert (snapshot.info["dimX"], snapshot.info["dimY"], snapshot.info["dimZ"]) == DIMS
            taken = regions(ctx, got, level_count)
            elements = sum((len(blob) - 12 * count) // 4 for blob, count in taken)
            assert snapshot.info["elements"] == elements and snapshot.info["deviceBytes"] == sum(len(blob) for blob, _ in taken)
            for name, write in writers(rect, level_count):
                write(ctx)
                assert ctx.read_region(0, *got) != taken[0], f"{name} changes nothing in {rect}"
                assert snapshot.restore() > 0.0
                assert_levels(regions(ctx, got, level_count), taken, f"{name}, restored, the rectangle")
                assert_levels(levels(ctx), before, f"{name}, restored, the whole world")
    finally:
        ctx.close()


# ---- 2. the relight loop ------------------------------------------------------------------------------------------------------------------------------

def test_the_relight_loop_needs_no_trip_to_the_host(dense_world):
    """snapshot A (unlit) -> light -> restore A -> brush -> snapshot B -> light: every level is the model's "brush, then light ONCE".  Without
    the restore the second bake shades the first one's colours."""
    solid, colour, ws = dense_world
    box = ((8, 0, 8), (120, 64, 120))
    p = lightmodel.params(*box, target=RGB, **SUN)
    strokes = [_sphere(CARVE, (60, 18, 60), 9), _box(FILL, (30, 0, 80), (33, 52, 86), 0xFF2040F0)]
    brushed = _brushed(solid, colour, strokes)
    want = model_world(DIMS, brushed[0], lightmodel.light(brushed[0], brushed[1], p))
    light = lambda c: c.world_light(*box, target=RGB, level_count=5, **SUN)
    ctx, twice = _context(ws), _context(ws)
    try:
        a = ctx.world_snapshot(0, 0, DIMS[0], DIMS[2], 5)
        light(ctx)
        a.restore()
        assert_levels(levels(ctx), [(ws.storage(k).tobytes(), ws.info(k).columnCount) for k in range(6)], "restored to the unlit world")
        ctx.brush(strokes, 5)
        b = ctx.world_snapshot(0, 0, DIMS[0], DIMS[2], 5)
        light(ctx)
        expected = [(want.storage(k).tobytes(), want.info(k).columnCount) for k in range(6)]
        assert_levels(levels(ctx), expected, "brush, then light once")
        b.restore()  # (and the unlit edited world is there for the next round)
        unlit = model_world(DIMS, *brushed)
        try:
            assert_levels(levels(ctx), [(unlit.storage(k).tobytes(), unlit.info(k).columnCount) for k in range(6)], "restored to the unlit edited world")
        finally:
            unlit.close()
        light(twice)
        twice.brush(strokes, 5)
        light(twice)
        assert twice.read_level(0) != expected[0], "lighting twice shades twice: the loop needs the restore"
    finally:
        want.close()
        ctx.close()
        twice.close()


# ---- 3. the arena moves under the snapshot ------------------------------------------------------------------------------------------------------------

def test_restore_behind_edits_and_a_compaction(dense_world):
    ctx = _context(dense_world[2])
    try:
        ctx.brush(STROKES[:3], 5)
        before = levels(ctx)
        snapshot = ctx.world_snapshot(*WHOLE, 5)
        for stroke in STROKES[3:]:
            ctx.brush([stroke], 5)
        assert ctx.edit_stats()[1] > 0, "block moves leave their old places behind"
        reclaimed, _ = ctx.compact()
        assert reclaimed > 0 and levels(ctx) != before
        snapshot.restore()
        assert_levels(levels(ctx), before, "restored behind the compaction")
        assert snapshot.diff()[1]["changedColumns"] == 0
    finally:
        ctx.close()


def test_restore_of_a_tall_terrain_into_a_compacted_arena_lays_it_out_again():
    """The terrain is captured, almost all of it is carved away and the arena compacted: the tails are sized for the little that is left (an
    eighth of it, 16384 colour slots at the least), so the restore cannot find room there -- the arena is laid out again and grows."""
    solid = _tall_solid()
    ws = _any_world(TALL, solid, _dense(solid))
    ctx = _context(ws)
    try:
        ctx.brush([_box(FILL, (4, 0, 4), (6, 250, 7), 0xFF102030)], 5)
        before, before_solid = levels(ctx), voxels(ctx, TALL)[0]
        snapshot = ctx.world_snapshot(0, 0, TALL[0], TALL[2], 5)
        assert int(before_solid.sum()) > 2 * 16384, "LOD 0 alone holds more colours than a compacted tail keeps spare"
        ctx.brush([_box(CARVE, (0, 1, 0), (TALL[0], TALL[1], TALL[2]))], 5)
        ctx.compact()
        used, abandoned, spare = ctx.edit_stats()
        assert abandoned == 0
        snapshot.restore()
        used_after, _, spare_after = ctx.edit_stats()
        assert used_after + spare_after > used + spare, "the arena has not been laid out again"
        assert_levels(levels(ctx), before, "the tall terrain restored")
    finally:
        ctx.close()
        ws.close()


def test_restore_behind_a_new_upload_of_the_same_world(dense_world):
    ws = dense_world[2]
    ctx = _context(ws)
    try:
        ctx.brush(STROKES[:6], 5)
        edited = levels(ctx)
        snapshot = ctx.world_snapshot(*WHOLE, 5)
        ctx.upload_world(ws)
        assert ctx.read_level(0) == (ws.storage(0).tobytes(), ws.info(0).columnCount), "the upload is back"
        snapshot.restore()
        assert_levels(levels(ctx), edited, "the edited state behind the upload")
        ctx.upload_world(ws)  # levels uploaded and not yet placed: the restore places them first
        snapshot.restore()
        assert_levels(levels(ctx), edited, "the edited state behind an upload nothing has placed yet")
    finally:
        ctx.close()


# ---- 4. stale levels -----------------------------------------------------------------------------------------------------------------------------------

def test_stale_levels_are_kept_stale(dense_world):
    """An edit at levelCount 0 leaves LOD 1 .. 5 behind; a snapshot at levelCount 3 holds them as they are.  After a full refresh the restore
    brings the stale LOD 1 .. 3 back and leaves the fresh LOD 4 and 5 alone -- nothing is rebuilt from LOD 0."""
    ctx = _context(dense_world[2])
    rect = (32, 32, 32, 32)
    try:
        ctx.brush([_box(FILL, (36, 0, 36), (44, 60, 44), 0xFF2040F0), _sphere(CARVE, (52, 14, 52), 7)], 0)
        stale = regions(ctx, rect, 3)
        snapshot = ctx.world_snapshot(*rect, 3)
        ctx.edit(*rect, *ctx.read_region(0, *rect), 5)  # the same columns, every level rebuilt over them
        fresh = levels(ctx)
        refreshed = regions(ctx, rect, 3)
        assert refreshed[0] == stale[0] and all(refreshed[k] != stale[k] for k in (1, 2, 3)), "the refresh changes LOD 1 .. 3 over the rectangle"
        snapshot.restore()
        assert_levels(regions(ctx, rect, 3), stale, "the stale levels")
        after = levels(ctx)
        assert after[4] == fresh[4] and after[5] == fresh[5], "the levels above levelCount stay as the refresh left them"
    finally:
        ctx.close()


# ---- 5. foreign columns ---------------------------------------------------------------------------------------------------------------------------------

def _with_foreign_group(ws, at):
    ctx = _context(ws)
    for _, args in group_plan(at, 3):
        ctx.set_columns(0, args["x"], args["z"], 1, 1, args["blob"], 1)
    return ctx


def test_foreign_columns_are_captured_restored_and_compare_equal(dense_world):
    at = (40, 68)
    ctx = _with_foreign_group(dense_world[2], at)
    try:
        solid, argb = voxels(ctx)
        assert_foreign(solid.transpose(0, 2, 1), argb.transpose(0, 2, 1), at)
        lo, hi = group_box(at)
        rect = (lo[0], lo[2], hi[0] - lo[0], hi[2] - lo[2])
        before = levels(ctx)
        snapshot = ctx.world_snapshot(*rect, 2)
        for flags in (0, IGNORE):
            changes, summary = snapshot.diff(flags)
            assert len(changes) == 0 and summary == {"changedColumns": 0, "changedVoxels": 0, "min": (0, 0, 0), "max": (0, 0, 0)}, \
                "the encoding differs and the voxels do not"
        ctx.brush([_box(FILL, (lo[0], 10, lo[2]), (hi[0], 50, hi[2]), 0xFF334455), _box(CARVE, (lo[0], 0, lo[2]), (hi[0], 4, hi[2]))], 2)
        now = voxels(ctx)
        changes, summary = snapshot.diff()
        want, want_summary = snapshotmodel.diff(cut((solid, argb), held(snapshot)), cut(now, held(snapshot)), held(snapshot)[:2])
        assert changes.tobytes() == want.tobytes() and summary == want_summary
        assert {tuple(c) for c in group_columns(at).values()} <= {(int(c["x"]), int(c["z"])) for c in changes}
        snapshot.restore()
        assert_levels(levels(ctx), before, "the foreign group restored")
        again = voxels(ctx)
        assert (again[0] == solid).all() and (again[1] == argb).all()
    finally:
        ctx.close()


# ---- 6. overlapping snapshots ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["a then b", "b then a"])
def test_overlapping_snapshots_the_later_restore_wins(dense_world, order):
    ctx = _context(dense_world[2])
    ra, rb = (16, 16, 48, 40), (40, 30, 50, 60)
    try:
        v0 = voxels(ctx)
        a = ctx.world_snapshot(*ra, 0)
        ctx.brush([_box(FILL, (30, 0, 20), (60, 50, 50), 0xFF808000)], 0)
        v1 = voxels(ctx)
        b = ctx.world_snapshot(*rb, 0)
        ctx.brush([_sphere(CARVE, (50, 20, 45), 25), _box(PAINT, (0, 0, 0), DIMS, 0xFF010203)], 0)
        want = [v.copy() for v in voxels(ctx)]
        for snapshot, rect, source in ((a, ra, v0), (b, rb, v1)) if order == "a then b" else ((b, rb, v1), (a, ra, v0)):
            snapshot.restore()
            x0, z0, sx, sz = rect
            for w, s in zip(want, source):
                w[x0:x0 + sx, z0:z0 + sz] = s[x0:x0 + sx, z0:z0 + sz]
        got = voxels(ctx)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), order
        once = ctx.read_level(0)
        (a if order == "b then a" else b).restore()  # the last one again: nothing changes
        assert ctx.read_level(0) == once
    finally:
        ctx.close()


# ---- 7, 8. the diff against the model ---------------------------------------------------------------------------------------------------------------------

def _diff_against_model(ctx, snapshot, before, label):
    """Both flags, the list, its order and the summary; a capacity of 0 with no list, a prefix, and the device variant's bytes."""
    rect = held(snapshot)
    now = voxels(ctx, (snapshot.info["dimX"], snapshot.info["dimY"], snapshot.info["dimZ"]))
    counts = []
    for flags in (0, IGNORE):
        want, want_summary = snapshotmodel.diff(cut(before, rect), cut(now, rect), rect[:2], flags)
        changes, summary = snapshot.diff(flags)
        assert summary == want_summary, f"{label}, flags {flags}: {summary} != {want_summary}"
        assert changes.tobytes() == want.tobytes(), f"{label}, flags {flags}: the list differs"
        none, summary = snapshot.diff(flags, capacity=0)
        assert len(none) == 0 and summary == want_summary, f"{label}: capacity 0"
        few = max(1, len(want) // 3)
        prefix, summary = snapshot.diff(flags, capacity=few)
        assert prefix.tobytes() == want[:few].tobytes() and summary == want_summary, f"{label}: a capacity of {few}"
        buffer = torch.full((len(want) + 2, 4), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert snapshot.diff_device(buffer.data_ptr(), len(want) + 1, flags) == want_summary
        torch.cuda.synchronize()
        back = buffer.cpu().numpy()
        assert back[:len(want)].tobytes() == want.tobytes() and (back[len(want):] == -7).all(), f"{label}: the device list"
        counts.append(want_summary["changedColumns"])
    return counts


def test_diff_matches_the_model_after_each_writer(dense_world):
    solid, colour, ws = dense_world
    ctx = _context(ws)
    try:
        ctx.brush([_box(FILL, (70, 0, 70), (72, DIMS[1], 72), 0xFF909090)], 5)  # a column that is solid up to dimY - 1
        before = [v.copy() for v in voxels(ctx)]
        base = levels(ctx)
        whole = ctx.world_snapshot(*WHOLE, 5)
        part = ctx.world_snapshot(*ODD, 2)
        assert before[0][70, 70].all() and before[0][10, 10, 0]
        steps = [
            ("nothing", lambda: None, (0, 0)),
            ("a one-voxel PAINT", lambda: ctx.brush([_box(PAINT, (60, 5, 60), (61, 6, 61), 0xFF123456)], 5), (1, 0)),
            ("one-voxel CARVEs at y = 0 and at y = dimY - 1", lambda: ctx.brush([_box(CARVE, (10, 0, 10), (11, 1, 11)),
                                                                                  _box(CARVE, (70, DIMS[1] - 1, 70), (71, DIMS[1], 71))], 5), (2, 2)),
            ("a sphere carve across x = 64 and z = 64", lambda: ctx.brush([_sphere(CARVE, (64, 16, 64), 11)], 5), None),
            ("settle", lambda: ctx.world_settle((0, 0, 0), DIMS, GROUND, 0, 5, 16), None),
            ("a bake", lambda: ctx.world_light((0, 0, 0), DIMS, target=RGB, level_count=5, **SUN), None),
        ]
        for label, step, expected in steps:
            step()
            counts = _diff_against_model(ctx, whole, before, label)
            _diff_against_model(ctx, part, before, label + ", the odd rectangle")
            if expected is not None:
                assert tuple(counts) == expected, (label, counts)
            elif label == "a bake":
                assert counts == [int(before[0].any(axis=2).sum()), 0], "every solid column changes colour, no voxel its solidity"
            else:
                assert counts[0] > 100 and counts[1] > 0, (label, counts)
            whole.restore()
            assert_levels(levels(ctx), base, f"{label}, restored")
            for snapshot in (whole, part):  # 8. a diff behind a restore finds nothing
                changes, summary = snapshot.diff()
                assert len(changes) == 0 and summary == {"changedColumns": 0, "changedVoxels": 0, "min": (0, 0, 0), "max": (0, 0, 0)}, label
    finally:
        ctx.close()


def test_diff_on_the_tall_and_the_sparse_world():
    """Colours kept column after column (the sparse world) and columns of 256 voxels with runs across the steps of the write kernels."""
    solid = _tall_solid()
    tall = _any_world(TALL, solid, _dense(solid))
    rng = np.random.default_rng(62)
    _, _, sparse = _pick_world(rng, DIMS, True)
    try:
        for ws, dims, strokes in ((tall, TALL, [_sphere(CARVE, (16, 100, 16), 40), _box(FILL, (3, 200, 3), (9, 256, 9), 0xFF445566), _box(PAINT, (20, 0, 0), (21, 256, 32), 0xFF0000FF)]),
                                  (sparse, DIMS, [_box(CARVE, (0, 20, 0), (128, 30, 128)), _box(FILL, (10, 0, 10), (20, 64, 20), 0xFF445566)])):
            ctx = _context(ws)
            try:
                before = [v.copy() for v in voxels(ctx, dims)]
                snapshot = ctx.world_snapshot(0, 0, dims[0], dims[2], 5)
                ctx.brush(strokes, 5)
                counts = _diff_against_model(ctx, snapshot, before, f"{dims}")
                assert counts[0] > 50 and counts[1] > 0
                snapshot.restore()
                assert snapshot.diff()[1]["changedColumns"] == 0
                now = voxels(ctx, dims)
                assert (now[0] == before[0]).all() and (now[1] == before[1]).all()
            finally:
                ctx.close()
    finally:
        tall.close()
        sparse.close()


# ---- 9. purity -------------------------------------------------------------------------------------------------------------------------------------------

def test_capture_and_diff_change_nothing(dense_world):
    ctx = _context(dense_world[2])
    try:
        ctx.brush(STROKES[:4], 5)
        before, stats = levels(ctx), ctx.edit_stats()
        with ctx.world_snapshot(*ODD, 5) as snapshot:
            assert snapshot.ms > 0.0
            assert (levels(ctx), ctx.edit_stats()) == (before, stats), "the capture"
            ctx.brush([STROKES[4]], 5)
            ctx.brush([_box(PAINT, (40, 0, 40), (80, 64, 80), 0xFF102030)], 5)
            edited, stats = levels(ctx), ctx.edit_stats()
            changes, summary = snapshot.diff()
            assert summary["changedColumns"] > 0 and snapshot.ms > 0.0
            assert (levels(ctx), ctx.edit_stats()) == (edited, stats), "the diff"
    finally:
        ctx.close()


# ---- 10. ordering against draws ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", BOTH_KERNELS, ids=[name for name, _ in BOTH_KERNELS])
def test_restore_is_ordered_on_the_stream(kernel):
    """An async draw, a restore, an async draw: the first buffer shows the edited world, the second the restored one, both as the oracle renders
    them."""
    from test_gpu_world_edit import _edited

    solid_a = _terrain()
    rect = (64, 32, 32, 32)
    solid_b, salt = _edited(solid_a, rect, kind=2)
    ws_a, ws_b = _world(solid_a), _world(solid_b, salt)
    fr = _frames(ws_a)[3]
    n_td, n_lr = scenes.used_rows(fr)
    ctx = _context(ws_a)
    try:
        ctx.set_resolution(W, H)
        snapshot = ctx.world_snapshot(*rect, 5)
        ctx.edit(*rect, *ws_b.extract_region(0, *rect), 5)
        ctx.set_latency_kernel(kernel[1])
        ctx.clear_raybuffers(0, CLEAR)
        ctx.clear_raybuffers(1, CLEAR)
        ctx.draw_segments(fr, 0, gpu.DRAW_ASYNC)
        snapshot.restore()
        ctx.draw_segments(fr, 1, gpu.DRAW_ASYNC)
        ctx.synchronize()
        first = (ctx.read_raybuffer(0, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(0, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        second = (ctx.read_raybuffer(1, gpu.RAYBUFFER_TOPDOWN)[:n_td], ctx.read_raybuffer(1, gpu.RAYBUFFER_LEFTRIGHT)[:n_lr])
        for ws, got, label in ((ws_b, first, "the draw before the restore"), (ws_a, second, "the draw after the restore")):
            o_td, o_lr, _ = O.draw_segments(ws, fr, W, H, clear=CLEAR)
            _assert_same(f"{kernel[0]}: {label}", got, (o_td[:n_td], o_lr[:n_lr]))
        assert not all((a == b).all() for a, b in zip(first, second)), "the restore must be visible in this frame"
    finally:
        ctx.close()
        ws_a.close()
        ws_b.close()


# ---- 11. errors --------------------------------------------------------------------------------------------------------------------------------------------

def test_every_rejection_leaves_the_world_as_it_was(dense_world):
    ws = dense_world[2]
    L = gpu.lib()
    ctx, other = _context(ws), _context(ws)
    solid = _tall_solid()
    tall = _any_world(TALL, solid, _dense(solid))
    small = host.WorldSet.from_voxels((16, 64, 16), *[np.arange(16, dtype=np.int32)] * 3, np.full(16, 0xFF112233, dtype=np.uint32))
    narrow, empty = _context(small), gpu.Context(0)
    try:
        ctx.brush(STROKES[:2], 5)
        other.brush([STROKES[2]], 5)
        snapshot = ctx.world_snapshot(*ODD, 2)
        ctx.brush([STROKES[3]], 5)
        before, before_other = levels(ctx), levels(other)
        change, summary = gpu.SnapshotChange(), gpu.SnapshotDiffSummary()
        address = gpu.C.addressof

        def refused(c, rc, pattern, code=-1):
            assert rc == code, (pattern, rc)
            assert pattern in L.cvx_last_error(c._h).decode(), (pattern, L.cvx_last_error(c._h).decode())

        # a snapshot of another context
        refused(other, L.cvx_world_snapshot_restore(other._h, snapshot._h, None), "another context")
        refused(other, L.cvx_world_snapshot_diff(other._h, snapshot._h, 0, address(change), 1, address(summary), None), "another context")
        # flags, capacities, NULLs
        with pytest.raises(gpu.CvxError, match="unknown flags bits 0x2"):
            snapshot.diff(flags=2)
        refused(ctx, L.cvx_world_snapshot_diff(ctx._h, snapshot._h, 0, address(change), -1, None, None), "changeCapacity -1")
        refused(ctx, L.cvx_world_snapshot_diff(ctx._h, snapshot._h, 0, None, 5, None, None), "changeCapacity 5 with no list")
        refused(ctx, L.cvx_world_snapshot_diff_device(ctx._h, snapshot._h, 0, None, 5, None, None), "changeCapacity 5 with no list")
        refused(ctx, L.cvx_world_snapshot_restore(ctx._h, None, None), "snap is NULL")
        refused(ctx, L.cvx_world_snapshot_diff(ctx._h, None, 0, None, 0, None, None), "snap is NULL")
        refused(ctx, L.cvx_world_snapshot(ctx._h, 0, 0, 8, 8, 0, None, None), "out is NULL")
        assert L.cvx_world_snapshot_restore(None, snapshot._h, None) == -1 and L.cvx_snapshot_info_get(None, None) == -1
        L.cvx_snapshot_destroy(None)
        # the capture's own
        for args, pattern in (((0, 0, 8, 8, 6), "levelCount 6"), ((0, 0, 8, 8, -1), "levelCount -1"), ((0, 0, 0, 8, 0), "does not meet"),
                              ((DIMS[0], 0, 8, 8, 0), "does not meet"), ((-8, 0, 8, 8, 0), "does not meet")):
            with pytest.raises(gpu.CvxError, match=pattern):
                ctx.world_snapshot(*args)
        with pytest.raises(gpu.CvxError, match="narrower than 2\\^levelCount = 32"):
            narrow.world_snapshot(0, 0, 16, 16, 5)
        narrow.world_snapshot(0, 0, 16, 16, 4).close()
        with pytest.raises(gpu.CvxError, match="LOD 0 has not been uploaded"):
            empty.world_snapshot(0, 0, 8, 8, 0)
        assert len(ctx.world_snapshot(-5, 120, 10, 100, 0).diff()[0]) == 0, "a rectangle that sticks out is clipped"
        assert levels(ctx) == before and levels(other) == before_other
        # a world of other dimensions
        ctx.upload_world(tall)
        for call in (snapshot.restore, snapshot.diff):
            with pytest.raises(gpu.CvxError, match="the snapshot was taken from one of 128 x 64 x 128"):
                call()
        assert ctx.read_level(0) == (tall.storage(0).tobytes(), tall.info(0).columnCount)
    finally:
        for c in (ctx, other, narrow, empty):
            c.close()
        tall.close()
        small.close()


def test_snapshots_close_with_their_context(dense_world):
    ctx = _context(dense_world[2])
    a, b = ctx.world_snapshot(*ONE, 0), ctx.world_snapshot(*ODD, 3)
    a.close()
    a.close()
    assert not a._h and ctx._snapshots == [b]
    ctx.close()
    assert not b._h and ctx._snapshots == []


def test_the_diff_list_around_the_count_in_both_forms():
    """The 8 x 8 columns in the middle of a 16 x 16 x 16 noise world after a carve through some of them, capacities 0 (no list), 1, found - 1,
    found and found + 1: the host and the device form give the same bytes, leave a list filled with a sentinel alone from min(found, capacity)
    on, and the summary is the same at every capacity."""
    dims, rect = (16, 16, 16), (4, 4, 8, 8)
    x, y, z = np.nonzero(np.random.default_rng(7).random(dims) < 0.5)
    ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), np.full(len(x), 0xFF204060, dtype=np.uint32), threads=2)
    ctx = _context(ws)
    try:
        before = voxels(ctx, dims)
        snapshot = ctx.world_snapshot(*rect, 0)
        ctx.brush([_box(CARVE, (5, 3, 5), (10, 12, 9))], 0)
        want, want_summary = snapshotmodel.diff(cut(before, rect), cut(voxels(ctx, dims), rect), rect[:2], 0)
        found = len(want)
        assert 2 < found < rect[2] * rect[3]
        for capacity in (0, 1, found - 1, found, found + 1):
            listed = min(capacity, found)
            on_host = np.full((found + 2, 4), -7, dtype=np.int32)
            on_device = torch.full((found + 2, 4), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            summary = snapshot._diff(gpu.lib().cvx_world_snapshot_diff, 0, on_host.ctypes.data if capacity else None, capacity)
            device_summary = snapshot.diff_device(on_device.data_ptr() if capacity else None, capacity, 0)
            torch.cuda.synchronize()
            back = on_device.cpu().numpy()
            assert summary == want_summary and device_summary == want_summary, capacity
            assert on_host[:listed].tobytes() == want[:listed].tobytes() and back[:listed].tobytes() == want[:listed].tobytes(), capacity
            assert (on_host[listed:] == -7).all() and (back[listed:] == -7).all(), f"capacity {capacity}: written behind entry {listed}"
    finally:
        ctx.close()
        ws.close()
