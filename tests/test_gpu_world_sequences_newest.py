"""GPU: cvx_world_lift_pieces and cvx_world_snapshot / _restore / _diff among the other world calls on one arena.

The call lists are those of tests/test_world_sequences_newest_cpu.py, which runs them on the models alone and asserts there what every case is
named for; here _Later of tests/test_gpu_world_sequences_later.py runs the same lists on a context beside the models.  lift COPY and the diff are
readers: the model's result exactly (host call and _device variant), no level changed, edit_stats() as before.  lift REMOVE and the restore are
writers: the model's volume becomes the state and LOD 0 .. 5 are compared with its host-built chain, byte for byte.
  A  the editor's loop on the terrain and the sparse world: snapshot, carve a tower free, lift REMOVE into device pools,
     cvx_world_place_models_device of the tower elsewhere, diff (the model's), restore, diff (empty)
  B  a lift REMOVE and a restore, each directly behind a compaction
  C  foreign columns (a split solid run, a split air run, shared colours, air runs alone) under lift COPY and the diff, then under lift REMOVE
     and the restore, at levelCount 0: LOD 1 .. 5 stay the upload's
  D  a lift REMOVE at levelCount 2: LOD 1 and 2 are the model's inside its rectangle, LOD 3 .. 5 the world's before it; a snapshot at
     levelCount 2 taken then, restored behind a bake of the whole world: LOD 0 .. 2 the snapshot's, LOD 3 .. 5 as the bake made them"""
import pytest

from test_gpu_world_copy import _assert_levels
from test_gpu_world_sequences_later import _Later
from test_world_sequences_later_cpu import assert_foreign, group_plan, refreshed, strokes_plan, work  # noqa: F401  (work: the fixture)
from test_world_sequences_newest_cpu import (BEHIND_A_COMPACTION, EDITORS_LOOP, NEWEST_READER_GROUP, NEWEST_WRITER_GROUP, PARTIAL_BAKE, PARTIAL_LIFT, PARTIAL_RECT,
                                             PARTIAL_RESTORE, PARTIAL_SNAPSHOT, PARTIAL_TOWER, foreign_reader_plan, foreign_writer_plan)

pytestmark = pytest.mark.gpu


class _Cached(_Later):
    """_Later whose check -- every level is the host-built chain of the model's world, byte for byte -- builds that chain once per state of the
    model: behind a reader (the capture, a diff, a lift COPY) and behind a compaction the volume is the one the step before was compared with."""
    built = None

    def check(self, label):
        if self.built is None or self.built[0] is not self.solid or self.built[1] is not self.colour:
            self.drop()
            self.built = (self.solid, self.colour, self.world())
        _assert_levels(self.ctx, self.built[2], self.built[2], 5, f"step {self.steps} ({label})")

    def drop(self):
        if self.built is not None:
            self.built[2].close()
            self.built = None

    def close(self):
        self.drop()
        super().close()


@pytest.mark.parametrize("sparse", [False, True])
def test_the_editors_loop_with_a_lift_and_a_snapshot(work, sparse):
    s = _Cached(31, work, sparse)
    try:
        start = [s.ctx.read_level(k) for k in range(6)]
        s.run(EDITORS_LOOP[:1])
        at_snapshot = [s.ctx.read_level(k) for k in range(6)]
        assert at_snapshot != start
        s.run(EDITORS_LOOP[1:])
        assert [s.ctx.read_level(k) for k in range(6)] == at_snapshot, "every level reads as it did when the snapshot was taken"
    finally:
        s.close()


@pytest.mark.parametrize("case", sorted(BEHIND_A_COMPACTION))
def test_the_newest_writers_directly_behind_a_compaction(work, case):
    s = _Cached(80, work)
    try:
        s.run(BEHIND_A_COMPACTION[case])
        s.render(f"compact, {case}", slice(1, 2))
    finally:
        s.close()


@pytest.mark.parametrize("at,plan", [(NEWEST_READER_GROUP, foreign_reader_plan()), (NEWEST_WRITER_GROUP, foreign_writer_plan())], ids=["readers", "writers"])
def test_foreign_columns_under_lift_and_snapshot(work, at, plan):
    """Everything at levelCount 0 on columns that are still as cvx_world_set_columns uploaded them: LOD 0 is the model's host-built world, LOD 1 .. 5
    stay the original world's."""
    s = _Later(100, work)
    old = s.world()
    s.default = lambda label: s.check_mixed(old, {}, label)
    try:
        s.run(group_plan(at, 70))
        assert_foreign(s.solid, s.colour, at)
        s.run(plan)
    finally:
        old.close()
        s.close()


def test_a_partial_lift_and_a_snapshot_of_stale_levels(work):
    s = _Later(61, work)
    try:
        s.run(strokes_plan(PARTIAL_TOWER, "tower stroke"))  # (every level refreshed: the case begins behind it)
    except BaseException:
        s.close()
        raise
    old = s.world()
    fresh = {1: [PARTIAL_RECT], 2: [PARTIAL_RECT]}
    s.default = lambda label: s.check_rects(old, fresh, label)
    baked = None
    try:
        s.run([PARTIAL_LIFT])
        assert refreshed(s.last, 2) == PARTIAL_RECT
        s.run([PARTIAL_SNAPSHOT])  # LOD 3 .. 5 over the rectangle are the old world's: the snapshot holds LOD 0 .. 2
        s.default = None
        s.run([PARTIAL_BAKE])
        baked = s.world()

        def restored(label):
            new = s.world()
            try:
                _assert_levels(s.ctx, new, baked, 2, label)  # LOD 0 .. 2: the snapshot's inside its rectangle; LOD 3 .. 5: as the bake made them
                x0, z0, sx, sz = (v >> 3 for v in s.taken()["stale"][2])
                assert new.extract_region(3, x0, z0, sx, sz) != baked.extract_region(3, x0, z0, sx, sz), "a rebuild of LOD 3 from the restored LOD 0 would differ"
            finally:
                new.close()

        s.default = restored
        s.run([PARTIAL_RESTORE])
    finally:
        if baked is not None:
            baked.close()
        old.close()
        s.close()
