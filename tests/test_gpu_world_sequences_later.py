"""GPU: the newer world calls one after another on one arena -- stamp, copy, cvx_world_write_heights, cvx_world_place_models,
cvx_world_write_voxels, cavities FILL, cvx_world_light_lamps and the brush's capsules and ellipsoids as writers; surface, distance, spread, nav,
cavities REPORT, read_voxels, read_heights and read_model as readers -- in the orders an editor uses them in, as tests/test_gpu_world_sequences.py
runs the older eight.

The call lists are those of tests/test_world_sequences_later_cpu.py, which runs them on the models alone and asserts there what every case is
named for; here _Later, a _Sequence, runs the same lists on a context beside the models.  A writer's model (the one its own test uses) becomes
the sequence's state and LOD 0 .. 5 are compared with it byte for byte (apply); a reader must return the model's result exactly, change no level
and leave edit_stats() as they were.  Everything is integers and bytes: no comparison has a tolerance.
  A  the editor's loop across a compaction, on the terrain, the sparse world and (the stepped writers) the 32 x 256 x 32 world
  B  each newer writer directly behind a compaction, and a terrain over the whole footprint that makes the arena be laid out again
  C  foreign columns (a split solid run, a split air run, shared colours, air runs alone) under every newer reader, then every newer writer
  D  heights, models, dense and cavities FILL at levelCount 2 in separate rectangles, a stamp at levelCount 5 over two of them, a full bake.
_Later also holds the calls of the two newest, cvx_world_lift_pieces and cvx_world_snapshot, whose cases are tests/test_gpu_world_sequences_newest.py."""
import numpy as np
import pytest
import torch

import cavitymodel
import lampmodel
from cpuvox_amd import gpu
from test_gpu_world_cavities import _report as _cavities_report
from test_gpu_world_dense import TALL, _any_world
from test_gpu_world_distance import _same
from test_gpu_world_lift import _assert_equals_model as _lift_equals
from test_gpu_world_lift import _device_call as _lift_device
from test_gpu_world_lift import _host_call as _lift_host
from test_gpu_world_nav import _check as _nav_check
from test_gpu_world_sequences import EVERYWHERE, SETUP, _Sequence
from test_gpu_world_snapshot import held as _held
from test_gpu_world_spread import _check as _spread_check
from test_gpu_world_surface import _surface
from test_world_light_cpu import model_world
from test_world_models_cpu import identity_at
from test_world_sequences_later_cpu import (BEHIND_A_COMPACTION, DIMS, LOOP_FIRST, LOOP_SECOND, LOOP_SETUP, PARTIAL, PARTIAL_LAMPS, PARTIAL_READS, PARTIAL_RECTS,
                                            PARTIAL_SETUP, PARTIAL_STAMP, READER_GROUPS, RELAYOUT, WRITER_GROUPS, Models, assert_foreign, group_plan, read_map, reader_plans, refreshed,
                                            relayout_need, rounded, sequence_world, strokes_plan, tall_loop, tall_world, work, writer_plans)  # noqa: F401  (work: the fixture)

pytestmark = pytest.mark.gpu


class _Later(_Sequence, Models):
    """_Sequence with one method per newer call; run(plan) makes the calls of a list.  `default`: the comparison behind every step where it is not
    "every level is the model's" (the cases with partial refreshes set it)."""
    dims = DIMS

    def __init__(self, seed, work, sparse=False):
        super().__init__(seed, sparse)
        self.work, self.last, self.before, self.default = work, None, None, None

    def run(self, plan):
        for call, args in plan:
            getattr(self, call)(**args)

    def apply(self, after, label, check=None):
        super().apply(after, label, check or self.default)

    def unchanged(self, stats, label):
        """Behind a reader: every level as before it, and the arena's statistics."""
        self.steps += 1
        (self.default or self.check)(label)
        assert self.ctx.edit_stats() == stats, f"{label}: a reader changed the arena's statistics"

    def check_rects(self, old, fresh, label):
        """check_mixed for several refreshed rectangles per level: LOD k is the model's inside the rectangles of fresh[k] (LOD-0 columns, aligned
        to the level; EVERYWHERE for LOD 0) and the world `old`'s outside them, compared cell by cell of the grid the rectangles' edges make."""
        new = self.world()
        try:
            for k in range(6):
                rects = [EVERYWHERE] if k == 0 else fresh.get(k, [])
                assert all(v % (1 << k) == 0 for r in rects for v in r), (k, rects)
                rects = [tuple(v >> k for v in r) for r in rects]
                xs = sorted({0, DIMS[0] >> k} | {v for r in rects for v in (r[0], r[0] + r[2])})
                zs = sorted({0, DIMS[2] >> k} | {v for r in rects for v in (r[1], r[1] + r[3])})
                for xa, xb in zip(xs, xs[1:]):
                    for za, zb in zip(zs, zs[1:]):
                        inside = any(r[0] <= xa and xb <= r[0] + r[2] and r[1] <= za and zb <= r[1] + r[3] for r in rects)
                        ws = new if inside else old
                        cell = (xa, za, xb - xa, zb - za)
                        assert self.ctx.read_region(k, *cell) == ws.extract_region(k, *cell), \
                            f"step {self.steps} ({label}): LOD {k}, columns {cell} {'inside' if inside else 'outside'} what has been refreshed"
        finally:
            new.close()

    # -- writers: the model's result becomes the state, every level is compared ---------------------------------------------------------------------
    def brush(self, strokes, label, level_count=5, check=None, overlaps=False):
        after = self.m_brush(strokes, label, overlaps)
        assert self.ctx.brush(strokes, level_count) > 0.0
        self.apply(after, label, check)

    def shapes(self, strokes, label, level_count=5, check=None, overlaps=False):
        after = self.m_shapes(strokes, label, overlaps)
        assert self.ctx.brush(strokes, level_count) > 0.0
        self.apply(after, label, check)

    def stamp(self, mesh, op, label, level_count=5, check=None, overlaps=False):
        after = self.m_stamp(mesh, op, label, overlaps)
        assert self.ctx.stamp_mesh(self.mesh(mesh), op, level_count) > 0.0
        self.apply(after, label, check)

    def copy(self, placements, label, level_count=5, check=None, overlaps=False):
        after = self.m_copy(placements, label, overlaps)
        assert self.ctx.copy(placements, level_count) > 0.0
        self.apply(after, label, check)

    def write_heights(self, write, label, level_count=5, check=None, overlaps=False):
        after = self.m_write_heights(write, label, overlaps)
        assert self.ctx.write_heights(*write, level_count) > 0.0
        self.apply(after, label, check)

    def place_models(self, models, instances, label, level_count=5, check=None, overlaps=False, order_matters=None):
        after = self.m_place_models(models, instances, label, overlaps, order_matters)
        assert self.ctx.place_models(models, instances, level_count) > 0.0
        self.apply(after, label, check)

    def write_voxels(self, write, label, level_count=5, check=None, overlaps=False):
        after = self.m_write_voxels(write, label, overlaps)
        assert self.ctx.write_voxels(*write, level_count) > 0.0
        self.apply(after, label, check)

    def fill_cavities(self, box, label, open_faces=0x3F, max_voxels=0, argb=0xFF123456, level_count=5, check=None, overlaps=False):
        after = self.m_fill_cavities(box, label, open_faces, max_voxels, argb, overlaps)
        want, want_summary, _ = cavitymodel.analyse(self.solid, *box, open_faces, max_voxels)
        got, summary, ms = self.ctx.world_cavities(*box, gpu.CAVITIES_FILL, open_faces, max_voxels, argb, level_count, capacity=8192)
        assert summary == want_summary and got.tobytes() == want[:8192].tobytes() and ms > 0.0, label
        self.apply(after, label, check)

    def lamps(self, p, lamps, label, level_count=5, check=None, overlaps=False):
        after = self.m_lamps(p, lamps, label, overlaps)
        ms = self.ctx.world_light_lamps(p["box_min"], p["box_max"], lampmodel.tuples(lamps), sun_dir=p["sun_dir"], sun_level=p["sun_level"], sun_range=p["sun_range"],
                                        sky_level=p["sky_level"], sky_range=p["sky_range"], floor_level=p["floor_level"], target=p["target"], level_count=level_count)
        assert ms > 0.0, label
        self.apply(after, label, check)

    def set_column(self, x, z, blob, label):
        after = self.m_set_column(x, z, blob, label)
        self.ctx.set_columns(0, x, z, 1, 1, blob, 1)
        self.apply(after, label)

    # -- readers: the model's result exactly, then nothing has changed -------------------------------------------------------------------------------
    def surface(self, box, label, solid_outside=0x04, flags=0, holds=None):
        self.m_surface(box, label, solid_outside, flags, holds)
        stats = self.ctx.edit_stats()
        _surface(self.ctx, self.solid, self.colour, *box, solid_outside, flags, label=label)
        self.unchanged(stats, label)

    def distance(self, box, label, R=8, mode=gpu.DISTANCE_TO_SOLID, solid_outside=0x04, holds=None):
        want = self.m_distance(box, label, R, mode, solid_outside, holds)
        stats = self.ctx.edit_stats()
        _same(self.ctx.distance(*box, R, mode, solid_outside), want, label)
        self.unchanged(stats, label)

    def spread(self, box, seeds, medium, label, step_faces=0x3F, max_steps=200, holds=None):
        self.m_spread(box, seeds, medium, label, step_faces, max_steps, holds)
        stats = self.ctx.edit_stats()
        _spread_check(self.ctx, self.solid, *box, seeds, medium, step_faces, max_steps, label)  # (the field and the totals)
        self.unchanged(stats, label)

    def nav(self, call, goals, label, holds=None):
        self.m_nav(call, goals, label, holds)
        stats = self.ctx.edit_stats()
        _nav_check(self.ctx, self.solid, call, goals, label)  # (every voxel position's step and the summary, the field built twice)
        self.unchanged(stats, label)

    def report_cavities(self, box, label, open_faces=0x3F, max_voxels=0, holds=None):
        self.m_report_cavities(box, label, open_faces, max_voxels, holds)
        stats = self.ctx.edit_stats()
        _cavities_report(self.ctx, self.solid, *box, open_faces, max_voxels, label=label)
        self.unchanged(stats, label)

    def read_voxels(self, box, label, holds=None):
        want = self.m_read_voxels(box, label, holds)
        stats = self.ctx.edit_stats()
        argb, mask = self.ctx.read_voxels(*box)
        assert (argb == want[0]).all() and (mask == want[1]).all(), label
        self.unchanged(stats, label)

    def read_heights(self, box, label, holds=None):
        want = self.m_read_heights(box, label, holds)
        stats = self.ctx.edit_stats()
        got = self.ctx.read_heights(*box, want_argb=True, want_bottoms=True)
        for g, w, what in zip(got, want, ("heights", "argb", "bottoms")):
            assert g.shape == w.shape and (g == w).all(), f"{label}: {what}"
        self.unchanged(stats, label)

    def read_model(self, src_min, size, transform, label, holds=None):
        want = self.m_read_model(src_min, size, transform, label, holds)
        stats = self.ctx.edit_stats()
        dst_size, instance = read_map(self.dims, src_min, size, transform)
        argb, mask = self.ctx.read_model(dst_size, instance.toModel)
        assert (argb == want[0]).all() and (mask == want[1]).all(), label
        self.unchanged(stats, label)


    # -- the newest calls (their plans: tests/test_world_sequences_newest_cpu.py) -------------------------------------------------------------------
    def lift_copy(self, box, anchors, label, capacity=8192, voxel_capacity=None, holds=None):
        """A reader: the list, the sums, the summary and both pools are the model's, through the host call and the _device variant."""
        want, room = self.m_lift_copy(box, anchors, label, capacity, voxel_capacity, holds)
        stats = self.ctx.edit_stats()
        _lift_equals(_lift_host(self.ctx, box, anchors, gpu.LIFT_COPY, capacity, room), want, room, label)
        pieces, summary, argb, mask = _lift_device(self.ctx, box, anchors, gpu.LIFT_COPY, capacity, room)
        _lift_equals((pieces, summary, argb.cpu().numpy().view(np.uint32), mask.cpu().numpy()), want, room, f"{label}, _device")
        self.unchanged(stats, label)

    def lift_remove(self, box, anchors, label, capacity=8192, voxel_capacity=None, level_count=5, check=None, overlaps=False, holds=None, device=False):
        """A writer.  device: into torch tensors, which place_lifted reads."""
        after = self.m_lift_remove(box, anchors, label, capacity=capacity, voxel_capacity=voxel_capacity, overlaps=overlaps, holds=holds)
        want, room = self.lift
        if device:
            pieces, summary, argb, mask = _lift_device(self.ctx, box, anchors, gpu.LIFT_REMOVE, capacity, room, level_count)
            self.pools = (pieces, argb, mask)
            got = (pieces, summary, argb.cpu().numpy().view(np.uint32), mask.cpu().numpy())
        else:
            got = _lift_host(self.ctx, box, anchors, gpu.LIFT_REMOVE, capacity, room, level_count)
        _lift_equals(got, want, room, label)
        self.apply(after, label, check)

    def place_lifted(self, offset, label, op=None, level_count=5, check=None, overlaps=False):
        """cvx_world_place_models_device of the largest piece of the last lift_remove, straight from its device pools."""
        after = self.m_place_lifted(offset, label, op, overlaps)
        pieces, argb, mask = self.pools
        k = self.largest_lifted()
        model = gpu.lifted_model(pieces, k, argb.data_ptr(), mask.data_ptr())
        at = tuple(int(pieces[k]["piece"]["min"][a]) + offset[a] for a in range(3))
        assert self.ctx.place_models_device([model], [identity_at(at, model[0], 0, gpu.BRUSH_FILL if op is None else op)], level_count) > 0.0
        self.apply(after, label, check)

    def snapshot(self, name, rect, label, levels=5):
        """The capture changes nothing; the handle is kept under `name` and closes with the context."""
        self.m_snapshot(name, rect, label, levels)
        self.ctx.read_level(0)  # (places a fresh upload's levels in the arena: edit_stats() counts them from here on)
        stats = self.ctx.edit_stats()
        handle = self.ctx.world_snapshot(*rect, levels)
        assert _held(handle) == self.taken()[name][2] and handle.info["levelCount"] == levels, label
        self.__dict__.setdefault("handles", {})[name] = handle
        self.unchanged(stats, label)

    def snapshot_diff(self, name, label, flags=0, holds=None):
        """A reader: the list and the summary are the model's, through the host call and the _device variant."""
        want, want_summary = self.m_snapshot_diff(name, label, flags, holds)
        stats = self.ctx.edit_stats()
        handle = self.handles[name]
        changes, summary = handle.diff(flags)
        assert summary == want_summary, f"{label}: {summary} != {want_summary}"
        assert changes.tobytes() == want.tobytes(), f"{label}: the list differs"
        buffer = torch.full((len(want) + 2, 4), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert handle.diff_device(buffer.data_ptr(), len(want) + 1, flags) == want_summary, f"{label}: _device"
        torch.cuda.synchronize()
        back = buffer.cpu().numpy()
        assert back[:len(want)].tobytes() == want.tobytes() and (back[len(want):] == -7).all(), f"{label}: the device list"
        self.unchanged(stats, label)

    def snapshot_restore(self, name, label, check=None, overlaps=False):
        after = self.m_snapshot_restore(name, label, overlaps)
        assert self.handles[name].restore() > 0.0
        self.apply(after, label, check)


class _LaterTall(_Later):
    """The same on the 32 x 256 x 32 world, whose columns the stepped writers walk in four steps."""
    dims = TALL

    def __init__(self, work):
        self.solid, self.colour = tall_world()
        self.ws = _any_world(TALL, self.solid, self.colour)
        self.ctx = gpu.Context(0)
        self.ctx.upload_world(self.ws)
        self.steps, self.work, self.last, self.before, self.default = 0, work, None, None, None

    def world(self):
        return model_world(TALL, self.solid, self.colour)


def _edited(seed, work):
    """test_gpu_world_sequences._edited as a _Later: six one-stroke brushes, every level compared after each."""
    s = _Later(seed, work)
    try:
        s.run(strokes_plan(SETUP, "setup stroke"))
        assert s.ctx.edit_stats()[1] > 0
    except BaseException:
        s.close()
        raise
    return s


# ---- A. the editor's loop across a compaction ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_the_editors_loop_across_a_compaction(work, sparse):
    """Six strokes; stamp, surface, copy, heights write, spread, models place, distance, dense write, nav, cavities FILL, lamps, read_heights,
    read_model twice, a capsule; a compaction; the same calls with other boxes and ops and an ellipsoid; a render through both kernels."""
    s = _Later(31, work, sparse)
    try:
        s.run(LOOP_SETUP + LOOP_FIRST)
        assert s.ctx.edit_stats()[1] > 0, "block moves leave their old places behind"
        s.compact("compaction")
        assert s.ctx.edit_stats()[1] == 0
        s.run(LOOP_SECOND)
        s.render("the editor's loop")
    finally:
        s.close()


def test_the_stepped_writers_across_a_compaction_in_the_tall_world(work):
    """Dense, heights, models and a capsule, each over columns the one before it edited, in a world four 64-voxel steps high; a compaction; the
    same with other ops."""
    s = _LaterTall(work)
    try:
        s.run(tall_loop(0))
        assert s.ctx.edit_stats()[1] > 0
        s.compact("compaction")
        assert s.ctx.edit_stats()[1] == 0
        s.run(tall_loop(1))
    finally:
        s.close()


# ---- B. each newer writer directly behind a compaction, and behind a relayout ---------------------------------------------------------------------------

@pytest.mark.parametrize("writer", sorted(BEHIND_A_COMPACTION))
def test_a_writer_directly_behind_a_compaction(work, writer):
    s = _edited(80, work)
    try:
        if writer != "cavities":  # (its list holds the compaction, between the shell and the FILL)
            s.compact("compaction")
        s.run(BEHIND_A_COMPACTION[writer])
        s.render(f"compact, {writer}", slice(1, 2))
    finally:
        s.close()


def test_a_terrain_that_does_not_fit_the_tails_lays_the_arena_out_again(work):
    """A REPLACE of the whole footprint with columns 44 .. 56 voxels deep, behind a compaction: the colours it needs (relayout_need, from the
    volumes) exceed everything the tails have left, so cvx_edit.hip's Relayout must run: the arena grows (used + spare, which no edit inside the
    tails changes), and the new tail of LOD 0's colours keeps the rule's headroom of 16384 slots at the least.  The models place, the spread and
    the read behind it see the new arena."""
    s = _edited(90, work)
    try:
        s.compact("compaction")
        edited = (sequence_world(90)[0] != s.solid).any(axis=1)  # the columns the setup edited
        old = s.solid
        used, abandoned, spare = s.ctx.edit_stats()
        assert abandoned == 0
        s.run(RELAYOUT[:1])
        need = 4 * relayout_need(old, s.solid, edited)
        assert need > spare, f"the write needs {need} bytes of colours, the tails have {spare} left"
        used_after, _, spare_after = s.ctx.edit_stats()
        assert used_after + spare_after > used + spare, "the arena has not been laid out again"
        assert used_after > used + need // 2 and spare_after >= 4 * 16384, (used, spare, used_after, spare_after)
        s.run(RELAYOUT[1:])
        s.render("behind the relayout", slice(1, 2))
    finally:
        s.close()


# ---- C. foreign columns ---------------------------------------------------------------------------------------------------------------------------------

def _uploaded(work, groups):
    """A sequence with one group of the four foreign columns per call, every level compared after every upload: (the sequence, the world as it
    was before, {level: the rectangle refreshed so far})."""
    s = _Later(100, work)
    old, fresh = s.world(), {}
    s.default = lambda label: s.check_mixed(old, fresh, label)
    try:
        for salt, at in enumerate(groups.values()):
            s.run(group_plan(at, 10 * salt))
            assert_foreign(s.solid, s.colour, at)
    except BaseException:
        old.close()
        s.close()
        raise
    return s, old, fresh


def test_foreign_columns_under_the_newer_readers(work):
    """Every reader over a group of its own that is still as cvx_world_set_columns uploaded it (the strokes beside a group are levelCount-0
    brushes whose rectangles hold none of its columns); set_columns and those brushes leave LOD 1 .. 5 as they were uploaded."""
    s, old, fresh = _uploaded(work, READER_GROUPS)
    try:
        for call, plan in reader_plans().items():
            s.run(plan)
    finally:
        old.close()
        s.close()


def test_foreign_columns_under_the_newer_writers(work):
    """Every writer over a fresh group, at levelCount 0 (cavities FILL: 2, and its rectangle of 4 x 4 columns): LOD 0 read back is the model's
    host-built world byte for byte -- the builder's encoding, split runs merged and shared colours unshared, and the other groups' columns with
    the voxels they were uploaded with --, LOD 1 .. 5 the original world's outside what has been refreshed."""
    s, old, fresh = _uploaded(work, WRITER_GROUPS)
    try:
        for call, plan in writer_plans().items():
            if call == "fill_cavities":
                at = WRITER_GROUPS[call]
                rect = rounded((at[0] + 1, at[1], 2, 1), 2)
                s.run(plan[:-1])
                fresh.update({1: rect, 2: rect})
                s.run(plan[-1:])
                assert refreshed(s.last, 2) == rect
            else:
                s.run(plan)
    finally:
        old.close()
        s.close()


# ---- D. a partial refresh by a newer writer, then a full one elsewhere ------------------------------------------------------------------------------------

def test_partial_refreshes_by_the_newer_writers_then_full_ones(work):
    """Heights, models, dense and cavities FILL at levelCount 2 in four separate rectangles; a stamp at levelCount 5 whose rounded rectangle holds the
    first, cuts the second and misses the others: LOD 1 and 2 are the model's inside the five rectangles, LOD 3 .. 5 inside the stamp's alone, and
    the ORIGINAL world's everywhere else, although LOD 0 has changed there.  distance and spread read LOD 0 alone; a bake of the whole world
    makes every level the model's."""
    s = _Later(61, work)
    try:
        s.run([PARTIAL_SETUP])  # (a sealed shell for the FILL to fill, every level refreshed: the case begins behind it)
    except BaseException:
        s.close()
        raise
    old, fresh = s.world(), {k: [] for k in range(1, 6)}
    s.default = lambda label: s.check_rects(old, fresh, label)
    try:
        for step, rect in zip(PARTIAL, PARTIAL_RECTS):
            for k in (1, 2):
                fresh[k].append(rounded(rect, 2))
            s.run([step])
        stamp = (0, 0, 64, 64)
        for k in range(1, 6):
            fresh[k].append(stamp)
        s.run([PARTIAL_STAMP])
        assert refreshed(s.last, 5) == stamp
        new = s.world()
        try:
            for k in (3, 4, 5):
                strips = [(64 >> k, 0, 64 >> k, 128 >> k), (0, 64 >> k, 64 >> k, 64 >> k)]
                assert any(new.extract_region(k, *r) != old.extract_region(k, *r) for r in strips), f"the partial writes changed columns of LOD {k} outside the stamp's rectangle"
        finally:
            new.close()
        s.run(PARTIAL_READS)
        s.default = None
        s.run([PARTIAL_LAMPS])
    finally:
        old.close()
        s.close()
