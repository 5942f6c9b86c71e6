"""GPU: the world calls one after another on one arena -- brush, cvx_world_pieces, cvx_world_settle, cvx_world_light, cvx_world_move, the pick,
cvx_world_set_columns and cvx_world_compact in the orders a host uses them in.

Each call has a GPU test of its own on a world that was uploaded fresh (or uploaded and brushed).  Here every call runs on what the others left:
block tables, colour bases and run lists that edits moved to the tails and a compaction laid out again, foreign columns nobody re-encoded yet,
levels a partial refresh left behind, and the scratch the pick and the move share.  There is no model of a sequence: the expected world is the
composition of the calls' dense models (pickmodel.apply_strokes, piecesmodel, settlemodel, lightmodel) on ONE (solid, colour) volume, turned into
a world on the host after every step; LOD 0 .. 5 read back are compared with it byte for byte (_assert_levels) after EVERY step -- every single
stroke of a setup included --, move results and piece lists as exact integers and bytes, picks as the pick test compares them, and the last world
is rendered through both kernels against the CPU oracle.  Where a step refreshes only some levels or only a rectangle (tests 3 and 4), every level
is still compared after it: with the model's world where the step refreshed it and with the world it must have left alone elsewhere.  Seeds and
call lists are fixed."""
import numpy as np
import pytest

import lightmodel
import piecesmodel
import settlemodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _box, _brushed, _check_picks, _sphere
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _context, _frames
from test_gpu_world_move import _device_move
from test_gpu_world_pieces import _report
from test_world_brush_cpu import _pick_world
from test_world_light_cpu import ALPHA, RGB, model_world
from test_world_move_cpu import bodies_to_array, model_results, world_bodies
from test_world_pieces_cpu import GROUND, OUTSIDE

pytestmark = pytest.mark.gpu

FILL, CARVE, PAINT = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT
REMOVE = gpu.PIECES_REMOVE
WHOLE = ((0, 0, 0), DIMS)
EVERYWHERE = (0, 0, DIMS[0], DIMS[2])
TOWER = 0xFF2040F0

# sixteen strokes, one call each: towers with colours of their own (deeper than their colour blocks: the blocks move to the tails), sphere carves
# into the terrain, and box carves through the towers that cut their tops loose
STROKES = [
    _box(FILL, (20, 0, 24), (24, 58, 30), TOWER), _box(FILL, (50, 0, 40), (53, 61, 47), TOWER), _box(FILL, (77, 0, 90), (83, 50, 93), TOWER),
    _sphere(CARVE, (40, 12, 44), 9), _box(FILL, (100, 0, 12), (104, 63, 15), TOWER), _box(FILL, (8, 0, 100), (13, 45, 108), TOWER),
    _box(CARVE, (16, 26, 20), (30, 29, 34)), _sphere(CARVE, (90, 20, 60), 7), _box(FILL, (60, 0, 70), (66, 40, 72), TOWER),
    _box(FILL, (110, 0, 110), (116, 56, 117), TOWER), _box(CARVE, (46, 30, 36), (58, 32, 50)), _sphere(CARVE, (70, 8, 20), 6),
    _box(FILL, (30, 0, 80), (33, 52, 86), TOWER), _box(FILL, (90, 0, 30), (96, 35, 33), TOWER), _box(CARVE, (96, 40, 8), (108, 44, 20)),
    _sphere(CARVE, (116, 28, 112), 5),
]


def _strips(rect, size):
    """The rectangles that cover a size[0] x size[1] grid without rect = (x0, z0, sx, sz)."""
    x0, z0, sx, sz = rect
    out = [(0, 0, x0, size[1]), (x0 + sx, 0, size[0] - x0 - sx, size[1]), (x0, 0, sx, z0), (x0, z0 + sz, sx, size[1] - z0 - sz)]
    return [r for r in out if r[2] > 0 and r[3] > 0]


class _Sequence:
    """One context and the model's volume side by side.  apply(after, label) makes `after` the model's state and compares every level: with the
    model's world (check), or, behind a step that refreshes only part of the levels, with the model's and an older world (check_mixed)."""

    def __init__(self, seed, sparse=False):
        self.solid, self.colour, self.ws = _pick_world(np.random.default_rng(seed), DIMS, sparse)
        self.ctx = _context(self.ws)
        self.steps = 0

    def close(self):
        self.ctx.close()
        self.ws.close()

    def world(self):
        return model_world(DIMS, self.solid, self.colour)

    def check(self, label):
        want = self.world()
        try:
            _assert_levels(self.ctx, want, want, 5, f"step {self.steps} ({label})")
        finally:
            want.close()

    def apply(self, after, label, check=None):
        """`check`: the comparison of this step where it is not "every level is the model's" (a partial refresh); it is never left out."""
        self.solid, self.colour = after
        self.steps += 1
        (check or self.check)(label)

    def check_mixed(self, old, fresh, label):
        """Every level after a step that refreshed only part of the world: LOD 0 is the model's; LOD k >= 1 is the model's where fresh[k] says
        so -- EVERYWHERE, or a rectangle (x0, z0, sizeX, sizeZ) in LOD-0 columns, aligned to the level -- and the world `old`'s everywhere else
        (fresh has no k: the whole level is old's)."""
        new = self.world()
        try:
            for k in range(6):
                rect = EVERYWHERE if k == 0 else fresh.get(k)
                if rect is None or rect == EVERYWHERE:
                    ws = old if rect is None else new
                    assert self.ctx.read_level(k) == (ws.storage(k).tobytes(), ws.info(k).columnCount), \
                        f"step {self.steps} ({label}): LOD {k} is not the {'old' if rect is None else 'new'} world's"
                    continue
                assert all(v % (1 << k) == 0 for v in rect), (k, rect)
                inner = tuple(v >> k for v in rect)
                assert self.ctx.read_region(k, *inner) == new.extract_region(k, *inner), f"step {self.steps} ({label}): LOD {k} inside the refreshed rectangle"
                for r in _strips(inner, (DIMS[0] >> k, DIMS[2] >> k)):
                    assert self.ctx.read_region(k, *r) == old.extract_region(k, *r), f"step {self.steps} ({label}): LOD {k} outside the refreshed rectangle, columns {r}"
        finally:
            new.close()

    # -- the calls, each against its model ----------------------------------------------------------------------------------------------------------
    def brush(self, strokes, label, level_count=5, check=None):
        assert self.ctx.brush(strokes, level_count) > 0.0
        self.apply(_brushed(self.solid, self.colour, strokes), label, check)

    def report(self, box, anchors, capacity, label):
        pieces, summary = _report(self.ctx, self.solid, *box, anchors, capacity=capacity, label=label)
        self.steps += 1
        self.check(label)  # (a REPORT changes nothing)
        return pieces, summary

    def remove(self, box, anchors, label, level_count=5):
        want, want_summary, _ = piecesmodel.analyse(self.solid, *box, anchors)
        pieces, summary, _ = self.ctx.world_pieces(*box, anchors, REMOVE, level_count=level_count, capacity=8192)
        assert summary == want_summary and pieces.tobytes() == want[:8192].tobytes(), label
        self.apply(piecesmodel.remove(self.solid, self.colour, *box, anchors), label)
        return summary

    def settle(self, box, anchors, label, max_drop=0, level_count=5, capacity=8192, check=None):
        """-> (summary, the model's pieces, their drops): what _settle of the settle test asserts, with the model run once."""
        want, want_drops, want_summary, after = settlemodel.settle(self.solid, self.colour, *box, anchors, max_drop)
        pieces, drops, summary, ms = self.ctx.world_settle(*box, anchors, max_drop, level_count=level_count, capacity=capacity)
        assert summary == want_summary, f"{label}: {summary} != {want_summary}"
        assert len(pieces) == len(drops) == min(capacity, len(want)), label
        assert pieces.tobytes() == want[:capacity].tobytes(), f"{label}: the list differs"
        assert drops.tolist() == want_drops[:capacity].tolist(), f"{label}: drops {drops.tolist()} != {want_drops[:capacity].tolist()}"
        assert ms > 0.0
        self.apply(after, label, check)
        return summary, want, want_drops

    def light(self, p, label, level_count=5, check=None):
        mask, _ = lightmodel.shades(self.solid, p)
        assert mask.any(), f"{label}: the box holds no voxel"
        ms = self.ctx.world_light(p["box_min"], p["box_max"], sun_dir=p["sun_dir"], sun_level=p["sun_level"], sun_range=p["sun_range"], sky_level=p["sky_level"],
                                  sky_range=p["sky_range"], floor_level=p["floor_level"], target=p["target"], level_count=level_count)
        assert ms > 0.0
        self.apply((self.solid, lightmodel.light(self.solid, self.colour, p)), label, check)

    def move(self, seed, count, label, lanes=(1, 64), distinct=None):
        """`count` bodies (the first `distinct` of world_bodies repeated, where given) through the host-array call and the device call."""
        few = world_bodies(seed, self.solid, False, distinct or count)
        want = model_results(self.solid, few, False)
        bodies = bodies_to_array(few)
        if distinct:
            bodies, want = np.tile(bodies, count // distinct), np.tile(want, count // distinct)
        assert len(bodies) == count
        routes = [("host arrays", self.ctx.world_move(bodies))] + [(f"lanesPerBody {g}", _device_move(self.ctx, bodies, g)) for g in lanes]
        for name, got in routes:
            bad = np.flatnonzero(got != want)
            assert not len(bad), f"{label}, {name}: {len(bad)} of {count} bodies differ; first {bodies[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"
        self.steps += 1
        return want

    def compact(self, label):
        reclaimed, ms = self.ctx.compact()
        assert reclaimed > 0 and ms > 0.0, f"{label}: nothing to compact"
        assert self.ctx.edit_stats()[1] == 0
        self.steps += 1
        self.check(label)

    def render(self, label, frames=slice(1, 3)):
        want = self.world()
        try:
            _check_world(self.ctx, want, _frames(want)[frames], label)
        finally:
            want.close()


def _sun(box, target=RGB, **kw):
    args = dict(sun_dir=(3, 4, 1), sun_level=150, sun_range=256, sky_level=80, sky_range=6, floor_level=25)
    args.update(kw)
    return lightmodel.params(*box, target=target, **args)


# ---- 1. the frame loop, across a compaction --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_the_frame_loop_across_a_compaction(sparse):
    """Sixteen one-stroke brushes; pieces, settle, light, move; a compaction; the same four with other boxes and parameters; one more brush.
    All six levels are compared after every one of these steps, the sixteen strokes included.
    sparse: the world keeps its colours column after column (deep columns far apart), and the towers stand among them."""
    s = _Sequence(31, sparse)
    try:
        for k, stroke in enumerate(STROKES):
            s.brush([stroke], f"stroke {k}")
        assert s.ctx.edit_stats()[1] > 0, "block moves leave their old places behind"
        _, _, floating = piecesmodel.analyse(s.solid, *WHOLE, GROUND)
        loose = int((floating & (s.colour == TOWER)).sum())
        assert loose > 500, f"the carves cut {loose} tower voxels loose"

        first = ((0, 0, 0), (100, 64, 128))
        pieces, _ = s.report(first, GROUND, 8192, "first report")
        assert len(pieces) >= 3, "the tower tops at least"
        summary, _, _ = s.settle(first, GROUND, "first settle")
        assert summary["fallenPieces"] > 0 and summary["fallenVoxels"] >= loose // 2
        s.light(_sun(((10, 0, 10), (110, 64, 120))), "first light")
        s.move(31, 1500, "first moves")

        s.compact("compaction")

        second = ((30, 0, -5), (140, 64, 126))
        s.report(second, GROUND | OUTSIDE, 300, "second report")
        s.brush([_box(CARVE, (104, 18, 100), (124, 21, 124))], "a carve after the compaction")  # cuts the last tower again, below its landed top
        summary, _, _ = s.settle(second, GROUND | OUTSIDE, "second settle", max_drop=7, capacity=3)
        assert summary["fallenPieces"] > 0, "the second settle moves something"
        s.light(_sun(((0, 5, 0), (128, 60, 128)), ALPHA, sun_dir=(-2, 5, -3), sky_range=3, sun_range=64), "second light")
        s.move(32, 1500, "second moves")
        s.brush([_sphere(FILL, (64, 30, 64), 8, 0xFF00C0FF), _sphere(PAINT, (40, 14, 44), 12, 0xFF808080)], "the last brush")
        s.render("the frame loop")
    finally:
        s.close()


# ---- 2. each writing call directly behind a compaction ----------------------------------------------------------------------------------------------

SETUP = [STROKES[k] for k in (0, 1, 3, 6, 10, 7)]  # towers, both carves that cut them, two craters


def _edited(seed):
    """A world after six one-stroke brushes, every level compared after each of them."""
    s = _Sequence(seed)
    try:
        for k, stroke in enumerate(SETUP):
            s.brush([stroke], f"setup stroke {k}")
        assert s.ctx.edit_stats()[1] > 0
    except BaseException:
        s.close()
        raise
    return s


def test_light_then_a_compaction_then_settle():
    s = _edited(41)
    try:
        s.light(_sun(((0, 0, 0), (80, 64, 80))), "light")
        s.compact("compaction")
        summary, _, _ = s.settle(WHOLE, GROUND, "settle behind the compaction")
        assert summary["fallenPieces"] > 0
        s.render("light, compact, settle", slice(1, 2))
    finally:
        s.close()


def test_settle_then_a_compaction_then_light():
    s = _edited(42)
    try:
        summary, _, _ = s.settle(((0, 0, 0), (90, 64, 90)), GROUND, "settle")
        assert summary["fallenPieces"] > 0
        s.compact("compaction")
        s.light(_sun(WHOLE, ALPHA, sky_range=8), "light behind the compaction")
        s.render("settle, compact, light", slice(1, 2))
    finally:
        s.close()


def test_remove_then_a_compaction_then_report():
    s = _edited(43)
    try:
        summary = s.remove(WHOLE, GROUND, "remove")
        assert summary["floatingPieces"] > 0
        s.compact("compaction")
        stats = s.ctx.edit_stats()
        pieces, summary = s.report(WHOLE, GROUND, 8192, "report behind the compaction")
        assert len(pieces) == 0 and summary["floatingPieces"] == 0 and summary["floatingVoxels"] == 0 and summary["anchoredPieces"] == 1
        assert s.ctx.edit_stats() == stats, "a REPORT leaves the arena alone"
        s.render("remove, compact, report", slice(1, 2))
    finally:
        s.close()


# ---- 3. foreign columns -----------------------------------------------------------------------------------------------------------------------------------

AIR = 0xFFFF
# (runs from the top as (colour index or AIR, length), colours): a column of DIMS[1] = 64 voxels with y 0 .. 19 and y 36 .. 45 solid
FOREIGN = {
    "split solid run": ([(AIR, 18), (0, 4), (4, 6), (AIR, 16), (10, 12), (22, 8)], 30),
    "split air run": ([(AIR, 10), (AIR, 8), (0, 10), (AIR, 9), (AIR, 7), (10, 20)], 30),
    "shared colours": ([(AIR, 18), (0, 10), (AIR, 16), (0, 20)], 20),   # the upper run shares the first ten colours of the lower one
}


def _foreign_blob(runs, colours, salt):
    """A sub-world blob of one column in the reference's layout: the header (offset, runs | worldMin << 16, worldMax), a guard, the runs, a guard,
    the colours."""
    assert sum(n for _, n in runs) == DIMS[1]
    words = [ci | (n << 16) for ci, n in runs]
    palette = [0xFF000000 | ((salt * 0x010305 + k * 0x070B0D) & 0xFFFFFF) for k in range(colours)]
    return np.array([0, len(runs) | (0 << 16), 46, 0, *words, 0, *palette], dtype=np.uint32).tobytes()


def test_settle_and_light_over_foreign_columns():
    """Two groups of the three foreign encodings (tests/test_world_readback_cpu.py::_foreign) uploaded with cvx_world_set_columns: a split solid
    run, a split air run, runs that share colours.  Beside every column stands a tower that touches its upper run; carving through the towers
    alone (levelCount 0: the rectangle is the towers' own, the foreign columns are not re-encoded) cuts the upper runs loose.  Settle then reads the
    first group as it was uploaded, and light the second; the model knows the columns only as decoded voxels (piecesmodel.decode_blob).

    set_columns and the level-0 brushes leave LOD 1 .. 5 as they were uploaded, and the settle refreshes its own rectangle of 32 x 32 columns
    alone, so the second group's levels stay stale until the light.  Every level is compared after every call all the same (check_mixed): LOD 0
    with the model's host-built world byte for byte (a read-back is in the builder's encoding whatever the column was uploaded in), LOD 1 .. 5
    with the model's world inside what has been refreshed so far and with the ORIGINAL world outside it."""
    s = _Sequence(51)
    old = s.world()
    groups = {"settled": [(70, 70), (75, 81), (85, 74)], "lit": [(10, 6), (17, 20), (25, 11)]}
    try:
        def level0(label):
            got = piecesmodel.decode_blob(s.ctx.read_level(0)[0], DIMS)
            assert (got[0] == s.solid).all() and (got[1] == s.colour).all(), f"{label}: LOD 0 differs from the model's"

        def untouched_above(label):
            s.check_mixed(old, {}, label)

        towers, cuts = [], []
        for g, (name, columns) in enumerate(groups.items()):
            for k, ((x, z), (kind, (runs, colours))) in enumerate(zip(columns, FOREIGN.items())):
                blob = _foreign_blob(runs, colours, 10 * g + k)
                s.ctx.set_columns(0, x, z, 1, 1, blob, 1)
                solid, colour = s.solid.copy(), s.colour.copy()
                solid[x, :, z], colour[x, :, z] = (a[0, :, 0] for a in piecesmodel.decode_blob(blob, (1, DIMS[1], 1)))
                assert solid[x, 36:46, z].all() and solid[x, 0:20, z].all() and solid[x, :, z].sum() == 30, kind
                s.apply((solid, colour), f"set_columns: {kind} at ({x}, {z})", untouched_above)
                towers.append(_box(FILL, (x + 1, 0, z), (x + 2, 46, z + 1), TOWER))
                cuts.append(_box(CARVE, (x + 1, 24, z), (x + 2, 28, z + 1)))
        assert len({int(c) for c in s.colour[25, 36:46, 11]} & {int(c) for c in s.colour[25, 0:20, 11]}) == 10, "the shared colours are shared"
        level0("set_columns")
        for k, stroke in enumerate(towers + cuts):  # (one call each: the rectangle of a call is the bounding box of its strokes)
            s.brush([stroke], f"towers and cuts, stroke {k}", level_count=0, check=untouched_above)
        level0("towers and cuts")
        _, _, floating = piecesmodel.analyse(s.solid, *WHOLE, GROUND)
        for x, z in groups["settled"] + groups["lit"]:
            assert floating[x, 36:46, z].all() and not floating[x, 0:20, z].any(), f"the upper run of column ({x}, {z}) hangs on its tower's top alone"

        # settle: the first group's block of 32 x 32 columns, read as uploaded.  What falls lies inside the box, so the rectangle the settle
        # refreshes is that block: inside it every level is the model's, outside it (the second group) LOD 1 .. 5 are still the original's
        box = ((64, 0, 64), (96, 64, 96))
        rect = (64, 64, 32, 32)
        summary, pieces, drops = s.settle(box, GROUND | OUTSIDE, "settle over foreign columns",
                                          check=lambda label: s.check_mixed(old, {k: rect for k in range(1, 6)}, label))
        assert summary["fallenPieces"] > 0 and piecesmodel.rectangle(pieces[drops > 0], DIMS, 5) == rect
        level0("settle over foreign columns")
        for x, z in groups["settled"]:
            assert s.solid[x, 32:42, z].all() and not s.solid[x, 42:46, z].any(), f"column ({x}, {z}) fell with its tower's top"
        # light: the whole world, the second group still as uploaded; after it every level is the model's
        s.light(_sun(WHOLE, sky_range=4), "light over foreign columns")
        s.light(_sun(((0, 0, 0), (40, 64, 40)), ALPHA), "light again: the columns are the builder's now")
        s.render("foreign columns", slice(1, 2))
    finally:
        old.close()
        s.close()


# ---- 4. a partial refresh, then a full one elsewhere ----------------------------------------------------------------------------------------------------------

def test_a_partial_refresh_then_a_full_one_elsewhere():
    """Settle with levelCount 2, then light with levelCount 5 over a box that overlaps the settle's rectangle partly: LOD 0 .. 2 are the new
    world's everywhere; LOD 3 .. 5 are the new world's inside the light's rounded rectangle and the ORIGINAL world's outside it, although LOD 0
    has changed there."""
    s = _Sequence(61)
    old = s.world()
    try:
        low = {1: EVERYWHERE, 2: EVERYWHERE}
        _, pieces, drops = s.settle(((0, 0, 0), (70, 64, 70)), GROUND, "settle, levelCount 2", level_count=2,
                                    check=lambda label: s.check_mixed(old, low, label))
        p = _sun(((40, 0, 40), (100, 64, 100)))
        rect = lightmodel.rectangle(p, DIMS, 5)
        assert rect == (32, 32, 96, 96)
        fallen = piecesmodel.rectangle(pieces[drops > 0], DIMS, 2)
        assert fallen[0] < rect[0] < fallen[0] + fallen[2] and fallen[1] < rect[1] < fallen[1] + fallen[3], "the two rectangles overlap partly"
        s.light(p, "light, levelCount 5", check=lambda label: s.check_mixed(old, {**low, 3: rect, 4: rect, 5: rect}, label))
        new = s.world()
        try:
            for k in (3, 4, 5):
                strips = _strips(tuple(v >> k for v in rect), (DIMS[0] >> k, DIMS[2] >> k))
                assert any(new.extract_region(k, *r) != old.extract_region(k, *r) for r in strips), \
                    f"the settle changed columns of LOD {k} outside the light's rectangle"
        finally:
            new.close()
    finally:
        old.close()
        s.close()


# ---- 5. the pick and the move share their scratch ----------------------------------------------------------------------------------------------------------------

def test_the_pick_and_the_move_share_their_scratch():
    """A small pick, a move whose bodies and results need more than the scratch the pick allocated (cvx_world_move frees it and allocates
    anew), a brush, a pick that fits into the scratch the move left, a small move.  The sizes are those of the records the calls copy
    (rays + hits, bodies + results), asserted below.  The 20 000 bodies are 2 500 distinct ones eight times over (the model moves a body in half a
    millisecond) and go through the host-array call, the one that uses the scratch."""
    per_ray = gpu.PICK_RAY_DTYPE.itemsize + gpu.PICK_HIT_DTYPE.itemsize
    per_body = gpu.MOVE_BODY_DTYPE.itemsize + gpu.MOVE_RESULT_DTYPE.itemsize
    assert 64 * per_ray < 4096 * per_ray <= 20000 * per_body, "the move grows the pick's scratch, and the second pick fits into it"
    s = _Sequence(71)
    try:
        rng = np.random.default_rng(72)
        _check_picks(s.ctx, s.solid, s.colour, rng, 64, "64 rays")
        s.move(71, 20000, "20 000 bodies", lanes=(), distinct=2500)
        s.brush([_sphere(CARVE, (64, 20, 64), 14), _box(FILL, (30, 0, 30), (40, 60, 40), 0xFF445566)], "a brush")
        _check_picks(s.ctx, s.solid, s.colour, rng, 4096, "4096 rays")
        s.move(73, 3, "3 bodies", lanes=(1,))
        s.check("after the picks and the moves")
    finally:
        s.close()
