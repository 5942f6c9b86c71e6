"""CPU: the call lists of tests/test_gpu_world_sequences_newest.py, run on the dense models alone.

The two newest world calls in the sequences of tests/test_world_sequences_later_cpu.py (whose Models class holds their models beside the others'):
cvx_world_lift_pieces as a reader (COPY) and as a writer (REMOVE), cvx_world_snapshot with its diff as a reader and its restore as a writer.
A plan is a list of (call, arguments); what a case is named for is asserted here from liftmodel, snapshotmodel and the volumes.
  A  the editor's loop: snapshot, carve a tower free, lift REMOVE, the lifted tower placed elsewhere, diff, restore, diff
  B  a lift REMOVE and a snapshot restore, each directly behind a compaction
  C  two more groups of foreign columns, under lift COPY and a snapshot diff, and under lift REMOVE and a restore
  D  a lift REMOVE at levelCount 2 in a rectangle of its own; a snapshot at levelCount 2 taken while LOD 3 .. 5 are stale, restored behind a bake"""
import numpy as np
import pytest

from test_gpu_world_brush import _box
from test_gpu_world_sequences import SETUP, STROKES
from test_world_light_cpu import RGB
from test_world_pieces_cpu import GROUND, OUTSIDE
from test_world_sequences_later_cpu import (CARVE, DIMS, FILL, PAINT, PARTIAL_RECTS, READER_GROUPS, WRITER_GROUPS, WRITERS, ModelRun, _columns, _overlap, _sun, assert_foreign,
                                            group_box, group_columns, group_plan, refreshed, rounded, sequence_world, strokes_plan, work)  # noqa: F401  (work: the fixture)

IGNORE_COLOUR = 1
TOWER = STROKES[0]    # a tower of 4 x 58 x 6 voxels from the ground
CUT = STROKES[6]      # the box carve through it, y 26 .. 28: the top, 4 x 29 x 6 = 696 voxels, comes loose
TOWER_TOP = ((20, 29, 24), (24, 58, 30))
LIFT_BOX = ((14, 0, 18), (34, 64, 38))


def _inside(box, voxel):
    return all(box[0][a] <= voxel[a] < box[1][a] for a in range(3))


def _tower_lifted(m, want):
    """holds of the lift over LIFT_BOX: a stored piece is the tower's top (or holds it), and nothing of it stays."""
    lift = want[0]
    stored = lift.pieces["piece"][:lift.summary["storedPieces"]]
    mine = [p for p in stored if all(p["min"][a] <= TOWER_TOP[0][a] and TOWER_TOP[1][a] <= p["max"][a] for a in range(3))]
    (x0, y0, z0), (x1, y1, z1) = TOWER_TOP
    return len(mine) == 1 and int(mine[0]["voxels"]) >= 696 and m.solid[x0:x1, y0:y1, z0:z1].all() and not lift.removed[0][x0:x1, y0:y1, z0:z1].any()


def _rect_of(box):
    return box[0][0], box[0][2], box[1][0] - box[0][0], box[1][2] - box[0][2]


# ---- A. the editor's loop -------------------------------------------------------------------------------------------------------------------------------

LOOP_OFFSET = (44, -9, 30)  # where the lifted tower goes: 44 columns along x, 30 along z, 9 voxels lower
LOOP_RECT = (8, 12, 96, 64)  # the snapshot: the tower, its new place and the columns between


def _both_places(m, want):
    """holds of the diff before the restore: changed columns where the tower stood and where it stands now."""
    cols = {(int(c["x"]), int(c["z"])) for c in want[0]}
    old = {(x, z) for x in range(20, 24) for z in range(24, 30)}
    new = {(x + LOOP_OFFSET[0], z + LOOP_OFFSET[2]) for x, z in old}
    return old <= cols and new & cols and want[1]["changedVoxels"] >= 2 * 696


EDITORS_LOOP = [
    ("brush", dict(strokes=[TOWER], label="a tower")),
    ("snapshot", dict(name="loop", rect=LOOP_RECT, levels=5, label="snapshot before the carve")),
    ("brush", dict(strokes=[CUT], label="a carve cuts the tower's top free")),
    ("lift_remove", dict(box=LIFT_BOX, anchors=GROUND | OUTSIDE, device=True, label="lift REMOVE into device pools", overlaps=True, holds=_tower_lifted)),
    ("place_lifted", dict(offset=LOOP_OFFSET, label="the lifted tower placed elsewhere from the device pools")),
    ("snapshot_diff", dict(name="loop", label="diff before the restore", holds=_both_places)),
    ("snapshot_diff", dict(name="loop", flags=IGNORE_COLOUR, label="diff before the restore, colours ignored", holds=_both_places)),
    ("snapshot_restore", dict(name="loop", label="restore", overlaps=True)),
    ("snapshot_diff", dict(name="loop", label="diff behind the restore", holds=lambda m, want: len(want[0]) == 0 and want[1]["changedColumns"] == 0)),
]


# ---- B. behind a compaction -------------------------------------------------------------------------------------------------------------------------------

def _moved_pieces(m, want):
    return want[0].summary["storedPieces"] >= 2


BEHIND_A_COMPACTION = {
    "lift": strokes_plan(SETUP, "setup stroke") + [
        ("compact", dict(label="compaction")),
        ("lift_remove", dict(box=((14, 0, 18), (60, 64, 52)), anchors=GROUND | OUTSIDE, label="lift REMOVE behind the compaction: the tops of both towers", holds=_moved_pieces)),
        ("snapshot", dict(name="after", rect=(0, 0, DIMS[0], DIMS[2]), levels=5, label="snapshot behind the lift")),
        ("snapshot_diff", dict(name="after", label="diff of the snapshot just taken", holds=lambda m, want: len(want[0]) == 0)),
    ],
    "restore": [("snapshot", dict(name="start", rect=(0, 0, DIMS[0], DIMS[2]), levels=5, label="snapshot of the upload"))] + strokes_plan(SETUP, "setup stroke") + [
        ("compact", dict(label="compaction")),
        ("snapshot_restore", dict(name="start", label="restore behind the compaction")),
        ("snapshot_diff", dict(name="start", label="diff behind the restore", holds=lambda m, want: len(want[0]) == 0)),
    ],
}


# ---- C. foreign columns -----------------------------------------------------------------------------------------------------------------------------------

NEWEST_READER_GROUP, NEWEST_WRITER_GROUP = (40, 48), (70, 108)  # beside READER_GROUPS (z = 8, 28) and WRITER_GROUPS (z = 68, 88)


def _upper_runs(at):
    """The columns of the group that hold voxels, and the box of their upper runs: y 36 .. 45, ten voxels of air above the lower ones."""
    return [c for kind, c in group_columns(at).items() if kind != "all air"]


def _lifts_the_split_run(at):
    """holds of a lift over the group's box: the upper runs float, one piece each, and the split solid run's holds the voxels of both of its runs
    (they touch at y = 42)."""
    def holds(m, want):
        lift = want[0]
        stored = lift.pieces["piece"][:lift.summary["storedPieces"]]
        for x, z in _upper_runs(at):
            mine = [p for p in stored if p["min"].tolist() == [x, 36, z] and p["max"].tolist() == [x + 1, 46, z + 1]]
            if len(mine) != 1 or int(mine[0]["voxels"]) != 10 or lift.removed[0][x, 36:46, z].any() or not lift.removed[0][x, 0:20, z].all():
                return False
        return True
    return holds


def _the_upper_runs_changed(at):
    def holds(m, want):
        got = {(int(c["x"]), int(c["z"])): (int(c["yMin"]), int(c["yMax"])) for c in want[0]}
        return all(got.get(c) == (36, 46) for c in _upper_runs(at)) and group_columns(at)["all air"] not in got
    return holds


def foreign_reader_plan(at=NEWEST_READER_GROUP):
    box = group_box(at)
    x, z = group_columns(at)["split air run"]
    beside = _box(PAINT, (x + 1, 0, z), (x + 2, 64, z + 1), 0xFF31D0A0)  # a levelCount-0 stroke whose rectangle holds no foreign column
    one = lambda m, want: [(int(c["x"]), int(c["z"])) for c in want[0]] == [(x + 1, z)]  # noqa: E731
    return [
        ("lift_copy", dict(box=box, anchors=GROUND, label="lift COPY over the foreign columns", holds=_lifts_the_split_run(at))),
        ("lift_copy", dict(box=box, anchors=GROUND, capacity=2, label="lift COPY, two pieces listed", holds=lambda m, want: len(want[0].pieces) == 2)),
        ("snapshot", dict(name="group", rect=_rect_of(box), levels=0, label="snapshot of the foreign columns")),
        ("snapshot_diff", dict(name="group", label="diff: the encoding differs, the voxels do not", holds=lambda m, want: len(want[0]) == 0)),
        ("brush", dict(strokes=[beside], level_count=0, label="a paint beside the split air run")),
        ("snapshot_diff", dict(name="group", label="diff behind the paint", holds=one)),
        ("snapshot_diff", dict(name="group", flags=IGNORE_COLOUR, label="diff behind the paint, colours ignored", holds=lambda m, want: len(want[0]) == 0)),
    ]


def foreign_writer_plan(at=NEWEST_WRITER_GROUP):
    box = group_box(at)
    return [
        ("snapshot", dict(name="group", rect=_rect_of(box), levels=0, label="snapshot of the foreign columns")),
        ("lift_remove", dict(box=box, anchors=GROUND, level_count=0, label="lift REMOVE of the upper runs", holds=_lifts_the_split_run(at))),
        ("snapshot_diff", dict(name="group", label="diff behind the REMOVE", holds=_the_upper_runs_changed(at))),
        ("snapshot_restore", dict(name="group", label="restore of the foreign columns")),
        ("snapshot_diff", dict(name="group", label="diff behind the restore", holds=lambda m, want: len(want[0]) == 0)),
        ("lift_copy", dict(box=box, anchors=GROUND, label="lift COPY over the restored columns", holds=_lifts_the_split_run(at))),
    ]


# ---- D. partial refreshes -----------------------------------------------------------------------------------------------------------------------------------

PARTIAL_TOWER = [_box(FILL, (70, 0, 20), (74, 58, 26), 0xFF2040F0), _box(CARVE, (66, 30, 16), (78, 33, 30))]  # every level refreshed: before the case begins
PARTIAL_BOX = ((64, 0, 14), (80, 64, 32))
PARTIAL_LIFT = ("lift_remove", dict(box=PARTIAL_BOX, anchors=GROUND | OUTSIDE, level_count=2, label="lift REMOVE, levelCount 2"))
PARTIAL_RECT = (64, 16, 12, 16)      # what the REMOVE refreshes at levelCount 2: its pieces' columns rounded to 4
PARTIAL_SNAPSHOT = ("snapshot", dict(name="stale", rect=(56, 8, 40, 40), levels=2, label="snapshot at levelCount 2, LOD 3 .. 5 stale"))
PARTIAL_BAKE = ("light", dict(p=_sun(((0, 0, 0), DIMS), RGB), label="a bake of the whole world"))
PARTIAL_RESTORE = ("snapshot_restore", dict(name="stale", label="restore behind the bake"))


# ---- the tests: every plan on the models alone ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_the_editors_loop_lifts_the_tower_and_comes_back(work, sparse):
    start = sequence_world(31, sparse)
    run = ModelRun(DIMS, *start, work)
    run.run(EDITORS_LOOP[:2])
    at_snapshot = run.solid, run.colour
    run.run(EDITORS_LOOP[2:4])
    lift = run.lift[0]
    k = run.largest_lifted()
    piece = lift.pieces["piece"][k]
    assert int(piece["voxels"]) >= 696 and all(piece["min"][a] <= TOWER_TOP[0][a] and TOWER_TOP[1][a] <= piece["max"][a] for a in range(3)), "the largest lifted piece is the tower's top"
    before = run.solid
    run.run(EDITORS_LOOP[4:5])
    new = tuple(slice(TOWER_TOP[0][a] + LOOP_OFFSET[a], TOWER_TOP[1][a] + LOOP_OFFSET[a]) for a in range(3))
    assert run.solid[new].all() and not before[new].all(), "the tower stands elsewhere"
    held = _columns(LOOP_RECT, DIMS)
    assert not (run.last & ~held).any() and not ((run.solid != at_snapshot[0]).any(axis=1) & ~held).any(), "everything since the snapshot lies inside it"
    run.run(EDITORS_LOOP[5:])
    assert (run.solid == at_snapshot[0]).all() and (run.colour == at_snapshot[1]).all(), "the restore brings the world of the snapshot back"
    assert [c for c, _ in EDITORS_LOOP] == ["brush", "snapshot", "brush", "lift_remove", "place_lifted", "snapshot_diff", "snapshot_diff", "snapshot_restore", "snapshot_diff"]


@pytest.mark.parametrize("case", sorted(BEHIND_A_COMPACTION))
def test_the_newest_writers_behind_a_compaction_change_the_edited_columns(work, case):
    run = ModelRun(DIMS, *sequence_world(80, False), work)
    moved = np.zeros((DIMS[0], DIMS[2]), dtype=bool)
    plan = BEHIND_A_COMPACTION[case]
    at = [c for c, _ in plan].index("compact")
    assert plan[at + 1][0] == {"lift": "lift_remove", "restore": "snapshot_restore"}[case], "the writer stands directly behind the compaction"
    for call, args in plan:
        run.run([(call, args)])
        if call == "brush":
            moved |= run.last
        elif call in WRITERS:
            assert (run.last & moved).any(), f"{args['label']} changes a column that a setup stroke moved"
    if case == "restore":
        start = sequence_world(80, False)
        assert (run.solid == start[0]).all() and (run.colour == start[1]).all()


def test_the_newest_foreign_groups_hold_what_they_are_named_for(work):
    taken = [c for at in list(READER_GROUPS.values()) + list(WRITER_GROUPS.values()) for c in group_columns(at).values()]
    for at, plan in ((NEWEST_READER_GROUP, foreign_reader_plan()), (NEWEST_WRITER_GROUP, foreign_writer_plan())):
        assert not any(_inside(group_box(at, margin=4), (x, 0, z)) for x, z in taken), "a group of its own, away from the others"
        run = ModelRun(DIMS, *sequence_world(100, False), work)
        run.run(group_plan(at, 70))
        assert_foreign(run.solid, run.colour, at)
        uploaded = run.solid.copy(), run.colour.copy()
        mine = np.zeros((DIMS[0], DIMS[2]), dtype=bool)
        for x, z in group_columns(at).values():
            mine[x, z] = True
        for call, args in plan:
            run.run([(call, args)])
            if call == "brush":
                assert not (_columns(refreshed(run.last, 0), DIMS) & mine).any(), "the stroke's rectangle holds no foreign column"
            if call == "lift_remove":
                assert (_columns(refreshed(run.last, 0), DIMS) & mine).sum() >= 3, "the REMOVE re-emits the foreign columns"
                x, z = group_columns(at)["split solid run"]
                assert run.solid[x, 0:20, z].all() and not run.solid[x, 20:, z].any(), "the lower runs of the split column stay"
        if at == NEWEST_WRITER_GROUP:
            assert (run.solid == uploaded[0]).all() and (run.colour == uploaded[1]).all(), "the restore brings the foreign columns' voxels back"


def test_the_partial_lift_and_the_stale_snapshot(work):
    run = ModelRun(DIMS, *sequence_world(61, False), work)
    run.run(strokes_plan(PARTIAL_TOWER, "tower stroke"))
    run.run([PARTIAL_LIFT])
    assert refreshed(run.last, 2) == PARTIAL_RECT and run.lift[0].summary["storedPieces"] >= 2
    assert not any(_overlap(PARTIAL_RECT, rounded(r, 2)) for r in PARTIAL_RECTS), "a rectangle of its own"
    assert any(v % 32 for v in PARTIAL_RECT), "LOD 3 .. 5 over it are not refreshed: they are stale when the snapshot is taken"
    w1 = run.solid, run.colour
    run.run([PARTIAL_SNAPSHOT])
    held = run.taken()["stale"][2]
    assert held == (56, 8, 40, 40) and _columns(PARTIAL_RECT, DIMS)[~_columns(held, DIMS)].sum() == 0, "the snapshot holds the REMOVE's rectangle"
    run.run([PARTIAL_BAKE])
    inside = _columns(held, DIMS)
    assert (run.last & inside).any() and (run.last & ~inside).any(), "the bake changes columns inside and outside the snapshot"
    w2 = run.solid, run.colour
    run.run([PARTIAL_RESTORE])
    assert (run.colour == np.where(inside[:, None, :], w1[1], w2[1])).all() and (run.solid == w1[0]).all(), "LOD 0: the snapshot's inside, the bake's outside"
