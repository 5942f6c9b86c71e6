"""GPU: letting the floating pieces of the device-resident world fall (cvx_world_settle).

Every result is compared with the dense model of tests/settlemodel.py, which moves the pieces of tests/piecesmodel.py down one voxel at a time by
the contract's step rule and knows nothing of the closed form the device computes: the totals, the list and the drops as exact integers and
bytes.  After a settle that moves something every level is read back against the host-built LOD chain of the model's result, the world is
rendered through both kernels against the CPU oracle, and a second settle with the same arguments must find nothing left to fall and leave
LOD 0 byte-identical."""
import numpy as np
import pytest

import piecesmodel
import settlemodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _box, _brushed, _dense, _world
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import DIMS, _check_world, _context, _frames
from test_world_brush_cpu import _pick_world
from test_world_pieces_cpu import GROUND, world_boxes

pytestmark = pytest.mark.gpu

FILL = gpu.BRUSH_FILL
WHOLE = ((0, 0, 0), DIMS)
RED, GREEN, BLUE, GREY = 0xFF0000FF, 0xFF00FF00, 0xFFFF0000, 0xFF888888


def _settle(ctx, solid, colour, box_min, box_max, anchors, max_drop=0, level_count=5, capacity=8192, label=""):
    """One settle against the model: the totals, the first `capacity` pieces byte for byte, their drops -> (the model's world after it, summary, drops)."""
    want, want_drops, want_summary, after = settlemodel.settle(solid, colour, box_min, box_max, anchors, max_drop)
    pieces, drops, summary, ms = ctx.world_settle(box_min, box_max, anchors, max_drop, level_count=level_count, capacity=capacity)
    assert summary == want_summary, f"{label}: {summary} != {want_summary}"
    assert len(pieces) == len(drops) == min(capacity, len(want)), label
    assert pieces.tobytes() == want[:capacity].tobytes(), f"{label}: the list differs"
    assert drops.tolist() == want_drops[:capacity].tolist(), f"{label}: drops {drops.tolist()} != {want_drops[:capacity].tolist()}"
    assert ms > 0.0
    return after, summary, want_drops


def _ws(solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(solid.shape, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def _verify(ctx, after, before, args, label, level_count=5, again=True):
    """The device world is the model's: every level, a render through both kernels, and (again) a second settle that moves nothing."""
    ws_after, ws_before = _ws(*after), _ws(*before)
    try:
        _assert_levels(ctx, ws_after, ws_before, level_count, label)
        if level_count == 5:
            _check_world(ctx, ws_after, _frames(ws_after)[1:2], label, fresh=False)
        if again:
            level0 = ctx.read_level(0)[0]
            stats = ctx.edit_stats()
            _, drops, summary, ms = ctx.world_settle(*args, level_count=level_count)
            assert summary["fallenPieces"] == 0 and summary["largestDrop"] == 0 and not drops.any() and ms > 0.0, f"{label}: a second settle moved something"
            assert ctx.read_level(0)[0] == level0 and ctx.edit_stats() == stats, f"{label}: a second settle touched the arena"
    finally:
        ws_after.close()
        ws_before.close()


def _floor(dims=DIMS):
    solid = np.zeros(dims, dtype=bool)
    solid[:, 0, :] = True
    return solid


@pytest.fixture()
def built():
    """build(strokes) -> (ctx, solid, colour): the floor plus the strokes, on the device through cvx_world_brush and in numpy."""
    made = []

    def build(strokes):
        solid = _floor()
        colour = _dense(solid)
        ws = _world(solid, colour)
        ctx = _context(ws)
        made.append((ctx, ws))
        ctx.brush(strokes, 5)
        solid, colour = _brushed(solid, colour, strokes)
        return ctx, solid, colour

    yield build
    for ctx, ws in made:
        ctx.close()
        ws.close()


# p and q hold each other: p's upper bar lies one voxel above q's upper bar (z = 50), q's lower bar one voxel above p's lower bar (z = 52); the poles
# that join each piece's two bars stand in z = 51 at opposite ends, so the two never share a face.  The floor stops p after 9, q rests on p after 10.
LINKS = [_box(FILL, (50, 20, 50), (55, 21, 51), RED), _box(FILL, (50, 10, 51), (51, 21, 52), RED), _box(FILL, (50, 10, 52), (55, 11, 53), RED),
         _box(FILL, (52, 18, 50), (57, 19, 51), GREEN), _box(FILL, (56, 12, 51), (57, 19, 52), GREEN), _box(FILL, (52, 12, 52), (57, 13, 53), GREEN)]


# ---- constructed cases ---------------------------------------------------------------------------------------------------------------------------

def test_a_slab_lands_on_the_floor_and_merges_with_it(built):
    ctx, solid, colour = built([_box(FILL, (20, 5, 20), (28, 6, 30), RED), _box(FILL, (20, 6, 20), (28, 7, 30), GREEN)])
    after, summary, drops = _settle(ctx, solid, colour, *WHOLE, GROUND, label="slab")
    assert drops.tolist() == [4] and summary == {"floatingPieces": 1, "floatingVoxels": 160, "fallenPieces": 1, "fallenVoxels": 160, "largestDrop": 4}
    assert after[0][22, 0:3, 22].all() and not after[0][22, 3:, 22].any()
    assert after[1][22, 1:3, 22].tolist() == [RED, GREEN] and after[1][22, 0, 22] == colour[22, 0, 22]  # one run of three voxels, colours in order
    _verify(ctx, after, (solid, colour), (*WHOLE, GROUND), "slab")


def test_the_column_that_stops_a_piece_is_not_its_lowest_one(built):
    """A table with one long leg: the leg ends 9 above the floor, but a static pole one voxel wide ends 4 below the table top in another column."""
    ctx, solid, colour = built([_box(FILL, (40, 20, 40), (48, 22, 48), RED), _box(FILL, (40, 10, 40), (41, 20, 41), RED), _box(FILL, (47, 1, 47), (48, 16, 48), GREY)])
    after, summary, drops = _settle(ctx, solid, colour, *WHOLE, GROUND, label="ledge")
    assert drops.tolist() == [4] and summary["fallenVoxels"] == 8 * 8 * 2 + 10
    _verify(ctx, after, (solid, colour), (*WHOLE, GROUND), "ledge")


@pytest.mark.parametrize("box,label", [(((56, 0, 56), (72, 128, 72)), "one workgroup relaxes the box"), (((0, 0, 0), (128, 128, 128)), "sweeps over several launches")])
def test_a_stack_of_twelve_slabs(box, label):
    """Slab k lies k voxels above slab k - 1 (slab 0 = the floor): drop_k = 1 + 2 + .. + k, and the relaxation needs a sweep per slab.  The world is
    128 voxels high here, not DIMS' 64: the gaps alone take 78.  The small box holds 448 solid runs, the whole world 16 576: on both sides of the
    4096 up to which a single workgroup relaxes the box."""
    dims = (128, 128, 128)
    solid = _floor(dims)
    y = 0
    for k in range(1, 13):
        y += k + 1
        solid[60:64, y, 60:64] = True
    assert y == 90
    colour = _dense(solid)
    ws = _ws(solid, colour)
    ctx = _context(ws)
    try:
        after, summary, drops = _settle(ctx, solid, colour, *box, GROUND, label=label)
        assert drops.tolist() == [k * (k + 1) // 2 for k in range(12, 0, -1)]  # (the list starts with the highest slab)
        assert after[0][61, 0:13, 61].all() and not after[0][61, 13:, 61].any()
        _verify(ctx, after, (solid, colour), (*box, GROUND), label)
    finally:
        ctx.close()
        ws.close()


def test_two_interlocked_pieces_fall_together(built):
    ctx, solid, colour = built(LINKS)
    after, summary, drops = _settle(ctx, solid, colour, *WHOLE, GROUND, label="links")
    assert drops.tolist() == [9, 10] and summary["floatingPieces"] == 2
    _verify(ctx, after, (solid, colour), (*WHOLE, GROUND), "links")


def test_pieces_that_rest_leave_the_arena_alone(built):
    """The box starts above the floor and nothing is anchored: the block stands on the (static) floor, and so does the arch over it, two voxels of
    air above the block.  (Inside one box a piece that TOUCHES another one from above is part of it; the arch is the nearest thing to a piece
    resting on a floating piece.)  Nothing moves: no edit."""
    ctx, solid, colour = built([_box(FILL, (30, 1, 30), (34, 4, 34), RED),
                                _box(FILL, (28, 1, 30), (29, 7, 34), GREEN), _box(FILL, (35, 1, 30), (36, 7, 34), GREEN), _box(FILL, (28, 6, 30), (36, 7, 34), GREEN)])
    box = ((0, 1, 0), DIMS)
    level0, stats = ctx.read_level(0)[0], ctx.edit_stats()
    after, summary, drops = _settle(ctx, solid, colour, *box, 0, label="resting")
    assert drops.tolist() == [0, 0] and summary["fallenPieces"] == 0 and summary["floatingPieces"] == 2
    assert ctx.read_level(0)[0] == level0 and ctx.edit_stats() == stats
    assert (after[0] == solid).all()


def test_nothing_anchored_over_the_whole_world(built):
    """The floor layer is a floating piece like the others; the world's bottom holds it (drop 0) and everything else settles onto it."""
    ctx, solid, colour = built(LINKS + [_box(FILL, (20, 5, 20), (28, 7, 30), BLUE), _box(FILL, (100, 30, 90), (101, 31, 91), GREY)])
    after, summary, drops = _settle(ctx, solid, colour, *WHOLE, 0, label="no anchors")
    assert summary["floatingPieces"] == 5 and summary["fallenPieces"] == 4 and drops[0] == 0 and summary["largestDrop"] == 29
    _verify(ctx, after, (solid, colour), (*WHOLE, 0), "no anchors")


def test_runs_cut_by_the_box(built):
    ctx, solid, colour = built([_box(FILL, (20, 1, 20), (24, 30, 24), RED), _box(FILL, (60, 20, 60), (64, 40, 64), GREEN)])
    # the box's bottom cuts the tower: its lower part stays right under the part inside, which holds still
    box = ((10, 10, 10), (40, 64, 40))
    level0 = ctx.read_level(0)[0]
    after, summary, drops = _settle(ctx, solid, colour, *box, 0, label="cut at the bottom")
    assert drops.tolist() == [0] and summary["floatingVoxels"] == 4 * 4 * 20 and ctx.read_level(0)[0] == level0
    # the box's top cuts the block: the part inside falls away from the part above it
    box = ((50, 0, 50), (70, 30, 70))
    after, summary, drops = _settle(ctx, solid, colour, *box, GROUND, label="cut at the top")
    assert drops.tolist() == [19] and summary["fallenVoxels"] == 4 * 4 * 10
    assert after[0][61, 1:11, 61].all() and not after[0][61, 11:30, 61].any() and after[0][61, 30:40, 61].all()
    _verify(ctx, after, (solid, colour), (*box, GROUND), "cut at the top")


def test_a_piece_lands_on_static_voxels_below_the_box(built):
    ctx, solid, colour = built([_box(FILL, (80, 1, 80), (84, 6, 84), GREY), _box(FILL, (80, 20, 80), (84, 24, 84), RED)])
    box = ((70, 10, 70), (90, 40, 90))
    after, summary, drops = _settle(ctx, solid, colour, *box, GROUND, label="below the box")
    assert drops.tolist() == [14]  # (down to the block under the box, four voxels past the box's bottom)
    _verify(ctx, after, (solid, colour), (*box, GROUND), "below the box")


def test_max_drop_steps_add_up(built):
    """k calls with maxDrop = 1 equal one call with maxDrop = k, and the unlimited call once k reaches the largest drop (10)."""
    strokes = LINKS + [_box(FILL, (20, 5, 20), (28, 7, 30), BLUE)]
    stepped, solid, colour = built(strokes)
    state = (solid, colour)
    level0 = {}
    for k in range(1, 11):
        state, summary, drops = _settle(stepped, *state, *WHOLE, GROUND, max_drop=1, label=f"step {k}")
        assert summary["fallenPieces"] == (3 if k <= 4 else 2 if k <= 9 else 1), k  # (what has landed is part of the ground: the list shrinks)
        level0[k] = stepped.read_level(0)[0]
    for k in (3, 10, 0):
        once, _, _ = built(strokes)
        after, summary, drops = _settle(once, solid, colour, *WHOLE, GROUND, max_drop=k, label=f"maxDrop {k}")
        assert drops.tolist() == ([3, 3, 3] if k == 3 else [4, 9, 10])
        assert once.read_level(0)[0] == level0[k or 10], f"maxDrop {k} against {k or 10} steps of one"
    assert (after[0] == state[0]).all() and (after[1] == state[1]).all()
    _verify(stepped, state, (solid, colour), (*WHOLE, GROUND), "ten steps of one")


def test_capacity_truncates_the_lists_only(built):
    strokes = [_box(FILL, (10 + 6 * k, 3 + (5 * k) % 11, 10 + 4 * (k % 3)), (13 + 6 * k, 5 + (5 * k) % 11, 12 + 4 * (k % 3)), 0xFF102030 + k) for k in range(8)]
    results = []
    for capacity in (0, 3, 8192, 8192):
        ctx, solid, colour = built(strokes)
        after, summary, drops = _settle(ctx, solid, colour, *WHOLE, GROUND, capacity=capacity, label=f"capacity {capacity}")
        assert summary["floatingPieces"] == 8 and summary["fallenPieces"] == 8
        results.append((ctx.read_level(0)[0], summary))
    assert all(r == results[0] for r in results[1:]), "the world or the totals depend on the capacity, or two contexts differ"
    _verify(ctx, after, (solid, colour), (*WHOLE, GROUND), "capacity")


def test_a_repeating_world_does_not_wrap_the_box(built):
    strokes = [_box(FILL, (2, 9, 3), (6, 12, 8), RED), _box(FILL, (120, 30, 122), (128, 33, 128), GREEN)]
    plain, solid, colour = built(strokes)
    repeating, _, _ = built(strokes)
    repeating.set_world_repeat(True)
    box = ((-10, 0, -10), (10, 64, 10))  # across the origin: only the tile's own corner, not the block at the far corner
    after, summary, drops = _settle(plain, solid, colour, *box, GROUND, label="bounded")
    again, summary_r, drops_r = _settle(repeating, solid, colour, *box, GROUND, label="repeating")
    assert drops.tolist() == drops_r.tolist() == [8] and summary == summary_r and repeating.read_level(0)[0] == plain.read_level(0)[0]
    assert after[0][125, 30:33, 125].all()
    repeating.set_world_repeat(False)  # (the oracle renders the bounded world)
    _verify(repeating, after, (solid, colour), (*box, GROUND), "repeating")


def test_a_partial_refresh_leaves_the_upper_levels(built):
    ctx, solid, colour = built([_box(FILL, (30, 10, 30), (36, 14, 36), RED), _box(FILL, (90, 10, 90), (96, 14, 96), BLUE)])
    box = ((0, 0, 0), (64, 64, 64))
    after, summary, drops = _settle(ctx, solid, colour, *box, GROUND, level_count=2, label="levelCount 2")
    assert drops.tolist() == [9] and after[0][92, 12, 92]
    _verify(ctx, after, (solid, colour), (*box, GROUND), "levelCount 2", level_count=2)


# ---- random worlds -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((32, 128, 32), True, 3)])
def test_settle_equals_the_model_on_random_worlds(dims, sparse, seed):
    """The worlds of the pieces test (records with 1 .. 3 runs, run-list columns, both colour layouts) through the real kernels: 10 random boxes,
    anchor masks, maxDrop values and capacities each (seed = the world's + 100), then the named boxes, every settle applied on top of the ones
    before it."""
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    state = (solid, np.where(solid, colour, 0).astype(colour.dtype))
    ctx = gpu.Context(0)
    moved = 0
    try:
        ctx.upload_world(ws)
        rng = np.random.default_rng(seed + 100)
        for k in range(10):
            while True:
                box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
                box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
                if piecesmodel.clip_box(dims, box_min, box_max) is not None:
                    break
            anchors, max_drop, capacity = int(rng.integers(0, 8)), int(rng.choice([0, 1, 3])), int(rng.choice([0, 3, 8192]))
            state, summary, _ = _settle(ctx, *state, box_min, box_max, anchors, max_drop, level_count=int(rng.integers(0, 5)), capacity=capacity,
                                        label=f"random box {k} {box_min} {box_max} anchors {anchors} maxDrop {max_drop}")
            moved += summary["fallenPieces"] > 0
            got = piecesmodel.decode_blob(ctx.read_level(0)[0], dims)
            assert (got[0] == state[0]).all() and (got[1] == state[1]).all(), f"random box {k}: the world differs from the model's"
        for name, (box_min, box_max, anchors) in world_boxes(dims).items():
            state, summary, _ = _settle(ctx, *state, box_min, box_max, anchors, level_count=4, label=name)  # (2^4 columns: the narrowest world)
            moved += summary["fallenPieces"] > 0
        got = piecesmodel.decode_blob(ctx.read_level(0)[0], dims)
        assert (got[0] == state[0]).all() and (got[1] == state[1]).all(), "after the named boxes"
    finally:
        ctx.close()
        ws.close()
    assert moved >= 2  # (over the 18 calls: at least one settle ran on a world that an earlier settle had edited)


# ---- errors --------------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_leave_the_world_alone(built):
    ctx, solid, colour = built([_box(FILL, (30, 10, 30), (36, 14, 36), RED)])
    level0 = ctx.read_level(0)[0]
    ok = dict(box_min=(0, 0, 0), box_max=(8, 8, 8), anchors=0)
    bad = [
        (dict(ok, box_max=(0, 8, 8)), "empty"), (dict(ok, box_min=(9, 0, 0)), "empty"),
        (dict(ok, box_min=(0, 64, 0), box_max=(8, 70, 8)), "outside the world"), (dict(ok, box_min=(-9, 0, 0), box_max=(0, 8, 8)), "outside the world"),
        (dict(ok, anchors=8), "anchors"), (dict(ok, anchors=-1), "anchors"), (dict(ok, max_drop=-1), "maxDrop"),
        (dict(ok, level_count=6), "levelCount"), (dict(ok, level_count=-1), "levelCount"), (dict(ok, capacity=-1), "pieceCapacity"),
    ]
    for kwargs, match in bad:
        with pytest.raises(gpu.CvxError, match=match):
            ctx.world_settle(**kwargs)
        assert ctx.read_level(0)[0] == level0, match
    lo, hi = np.zeros(3, dtype=np.int32), np.full(3, 8, dtype=np.int32)
    L = gpu.lib()
    assert L.cvx_world_settle(ctx._h, None, hi.ctypes.data, 0, 0, 5, None, None, 0, None, None) == -1
    assert L.cvx_world_settle(ctx._h, lo.ctypes.data, hi.ctypes.data, 0, 0, 5, None, None, 2, None, None) == -1  # a capacity without a list
    assert ctx.read_level(0)[0] == level0
    empty = gpu.Context(0)
    try:
        with pytest.raises(gpu.CvxError, match="not been uploaded"):
            empty.world_settle((0, 0, 0), (8, 8, 8), 0)
    finally:
        empty.close()
    # NULL drops and summary with a list: valid
    pieces = np.zeros(4, dtype=gpu.PIECE_DTYPE)
    assert L.cvx_world_settle(ctx._h, lo.ctypes.data, np.array(DIMS, dtype=np.int32).ctypes.data, GROUND, 0, 5, pieces.ctypes.data, None, 4, None, None) == 0
    assert pieces[0]["min"].tolist() == [30, 10, 30]
    after = settlemodel.settle(solid, colour, *WHOLE, GROUND)[3]
    _verify(ctx, after, (solid, colour), (*WHOLE, GROUND), "after the call without drops")
