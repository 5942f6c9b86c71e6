"""GPU: the floating pieces of the device-resident world as models with mass moments (cvx_world_lift_pieces, include/cpuvox_gpu_lift.h).

Every result is compared byte for byte with the dense model of tests/liftmodel.py (piecesmodel.analyse and scipy.ndimage.label on the numpy
volume the world was built from): the list with its offsets and sums, the summary and both pools.  Every COPY call is made twice with identical
bytes, and a third time through the _device variant into torch tensors.  Pools are pre-filled with a sentinel: what lies at and beyond
storedVoxels stays untouched.  REMOVE is checked by reading every level back against the host-built LOD chain of the model's result, by
rendering through both kernels against the CPU oracle, and by a final REPORT that finds nothing floating; the round trip puts every lifted
piece back with cvx_world_place_models_device and finds the original world."""
import numpy as np
import pytest
import torch

import liftmodel
import piecesmodel
from cpuvox_amd import gpu, host
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import _check_world, _context, _frames
from test_world_brush_cpu import _pick_world
from test_world_lift_cpu import interlocked
from test_world_pieces_cpu import GROUND, LARGEST, OUTSIDE, world_boxes

pytestmark = pytest.mark.gpu

COPY, REMOVE = gpu.LIFT_COPY, gpu.LIFT_REMOVE
DIMS = (64, 128, 64)
WHOLE = ((0, 0, 0), DIMS)
SENTINEL, SENTINEL_BYTE = 0xA5A5A5A5, 0xA5
SPARE = 37  # elements of every pool behind the capacity


def _colours(solid):
    x, y, z = np.nonzero(solid)
    colour = np.zeros(solid.shape, dtype=np.uint32)
    colour[x, y, z] = 0xFF000000 | (x << 16) | (y << 8) | z
    return colour


def _world_of(solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(solid.shape, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def _floor(dims=DIMS):
    solid = np.zeros(dims, dtype=bool)
    solid[:, 0, :] = True
    return solid


@pytest.fixture()
def uploaded():
    """upload(solid, colour) -> ctx: the world built on the host from the dense arrays."""
    made = []

    def upload(solid, colour):
        ws = _world_of(solid, colour)
        ctx = _context(ws)
        made.append((ctx, ws))
        return ctx

    yield upload
    for ctx, ws in made:
        ctx.close()
        ws.close()


def _host_call(ctx, box, anchors, op, capacity, voxel_capacity, level_count=5):
    """One host call with sentinel-filled pools -> (pieces, summary, argb, solid)."""
    argb = np.full(voxel_capacity + SPARE, SENTINEL, dtype=np.uint32)
    solid = np.full(voxel_capacity + SPARE, SENTINEL_BYTE, dtype=np.uint8)
    pieces, summary, argb, solid, ms = ctx.world_lift_pieces(*box, anchors, op, level_count, capacity, voxel_capacity, argb=argb, solid=solid)
    assert ms > 0.0
    return pieces, summary, argb, solid


def _device_call(ctx, box, anchors, op, capacity, voxel_capacity, level_count=5):
    argb = torch.full((voxel_capacity + SPARE,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    solid = torch.full((voxel_capacity + SPARE,), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pieces, summary, ms = ctx.world_lift_pieces_device(*box, anchors, argb, solid, op, level_count, capacity, voxel_capacity)
    assert ms > 0.0
    return pieces, summary, argb, solid


def _assert_equals_model(got, want, voxel_capacity, label):
    pieces, summary, argb, solid = got
    assert summary == want.summary, f"{label}: {summary} != {want.summary}"
    assert pieces.tobytes() == want.pieces.tobytes(), f"{label}: the list differs, first at piece {int(np.argmax(pieces != want.pieces)) if len(pieces) == len(want.pieces) else -1}"
    stored = want.summary["storedVoxels"]
    assert stored <= voxel_capacity
    assert argb[:stored].tobytes() == want.argb.tobytes(), f"{label}: the colour pool differs at element {int(np.argmax(argb[:stored] != want.argb))}"
    assert solid[:stored].tobytes() == want.solid.tobytes(), f"{label}: the mask pool differs at element {int(np.argmax(solid[:stored] != want.solid))}"
    assert (argb[stored:] == SENTINEL).all() and (solid[stored:] == SENTINEL_BYTE).all(), f"{label}: something was written at or beyond storedVoxels"


def _copy(ctx, solid, colour, box, anchors, capacity=8192, voxel_capacity=None, label="", device=True):
    """COPY against the model: twice on the host (identical bytes) and once through the _device variant.  voxel_capacity None: exactly what the
    listed pieces need."""
    if voxel_capacity is None:
        voxel_capacity = liftmodel.lift(solid, colour, *box, anchors, capacity, 1 << 62).summary["storedVoxels"]
    want = liftmodel.lift(solid, colour, *box, anchors, capacity, voxel_capacity)
    first = _host_call(ctx, box, anchors, COPY, capacity, voxel_capacity)
    _assert_equals_model(first, want, voxel_capacity, label)
    again = _host_call(ctx, box, anchors, COPY, capacity, voxel_capacity)
    assert again[1] == first[1] and all(a.tobytes() == b.tobytes() for a, b in zip(again[:1] + again[2:], first[:1] + first[2:])), f"{label}: two calls differ"
    if device:
        pieces, summary, argb, mask = _device_call(ctx, box, anchors, COPY, capacity, voxel_capacity)
        on_host = (pieces, summary, argb.cpu().numpy().view(np.uint32), mask.cpu().numpy())
        assert summary == first[1] and all(a.tobytes() == b.tobytes() for a, b in zip(on_host[:1] + on_host[2:], first[:1] + first[2:])), f"{label}: _device differs"
    return first[0], first[1], want


# ---- random worlds -----------------------------------------------------------------------------------------------------------------------------------

def _split_run_column(ctx, solid, colour, x, z):
    """A foreign column (cvx_world_set_columns) whose encoding cuts one solid span, y 10 .. 29, into two adjacent runs."""
    dy = solid.shape[1]
    runs = [0xFFFF | ((dy - 30) << 16), 0 | (10 << 16), 10 | (10 << 16), 0xFFFF | (10 << 16)]  # from the top; colour index = the solid voxels above
    blob = np.array([0, len(runs) | (10 << 16), 30, 0, *runs, 0, *[0xFF000000 | (k * 0x010203) for k in range(20)]], dtype=np.uint32).tobytes()
    ctx.set_columns(0, x, z, 1, 1, blob, 1)
    solid[x, :, z], colour[x, :, z] = False, 0
    solid[x, 10:30, z] = True
    colour[x, 10:30, z] = [0xFF000000 | ((29 - y) * 0x010203) for y in range(10, 30)]


@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((32, 128, 32), True, 3)])
def test_copy_equals_the_model_on_random_worlds(dims, sparse, seed):
    """The worlds of the CPU tests (records with 1 .. 3 runs, run-list columns, both colour layouts) with two foreign split-run columns each,
    through the real kernels: the named boxes and 20 random boxes and anchor masks each (boxes that cut runs at y0 / y1 among them), the
    capacities drawn from {0, exact, ample}."""
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        _split_run_column(ctx, solid, colour, 5, 7)
        _split_run_column(ctx, solid, colour, dims[0] - 2, dims[2] - 3)
        stored = 0
        for name, (box_min, box_max, anchors) in world_boxes(dims).items():
            _, summary, _ = _copy(ctx, solid, colour, (box_min, box_max), anchors, label=name)
            stored += summary["storedPieces"]
        assert stored > 0
        rng = np.random.default_rng(seed + 200)
        cut = 0
        for k in range(20):
            box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
            box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
            if piecesmodel.clip_box(dims, box_min, box_max) is None:
                box_min, box_max = [0, 0, 0], [max(v, 1) for v in box_max]
            cut += 0 < box_min[1] or box_max[1] < dims[1]
            anchors = int(rng.integers(0, 8))
            needed = liftmodel.lift(solid, colour, box_min, box_max, anchors, 8192, 0).summary["neededVoxels"]
            voxel_capacity = [0, needed, needed + 1000][int(rng.integers(0, 3))]
            _copy(ctx, solid, colour, (box_min, box_max), anchors, capacity=int(rng.choice([0, 3, 8192])), voxel_capacity=voxel_capacity,
                  label=f"random box {k}", device=k % 4 == 0)
        assert cut >= 10
    finally:
        ctx.close()
        ws.close()


# ---- constructed cases -------------------------------------------------------------------------------------------------------------------------------

def test_interlocked_pieces_hold_their_own_voxels_only(uploaded):
    """A U-frame and a bar through its opening: the bar's box lies across the frame's, and neither array holds a voxel of the other."""
    solid, colour = interlocked()
    ctx = uploaded(solid, colour)
    whole = ((0, 0, 0), solid.shape)
    pieces, summary, want = _copy(ctx, solid, colour, whole, GROUND, label="interlocked")
    assert summary["floatingPieces"] == 2 == summary["storedPieces"] and summary["storedVoxels"] == 360 + 288
    _, _, argb, mask = _host_call(ctx, whole, GROUND, COPY, 8, 648)
    size, frame_argb, frame_solid = gpu.lifted_model(pieces, 0, argb, mask)
    assert size == (12, 10, 3) and int(frame_solid.sum()) == int(pieces[0]["piece"]["voxels"]) and not frame_solid[3:9, :, 3:5].any()
    size, bar_argb, bar_solid = gpu.lifted_model(pieces, 1, argb, mask)
    assert size == (6, 2, 24) and bar_solid.all() and bar_argb[0, 0, 0] == colour[11, 13, 4] and bar_argb[5, 23, 1] == colour[16, 14, 27]
    # the mass properties of the bar: a 6 x 2 x 24 cuboid
    centre, inertia = gpu.lifted_piece_mass(pieces[1])
    assert centre.tolist() == [14.0, 14.0, 16.0]
    n = 288.0
    assert np.allclose(inertia, [n * (2 * 2 + 24 * 24 + 2) / 12, n * (6 * 6 + 24 * 24 + 2) / 12, n * (6 * 6 + 2 * 2 + 2) / 12, 0, 0, 0], rtol=1e-12, atol=1e-9)
    # the two pieces in boxes of their own, anchored by nothing
    _copy(ctx, solid, colour, ((8, 10, 14), (20, 20, 17)), 0, label="the frame's box: the frame and a slice of the bar")


def test_node_lengths_around_the_64_voxel_step_of_the_write_loop(uploaded):
    """Floating pillars of 1, 64, 65 and 100 voxels in a 128-high world, every voxel a colour of its own."""
    solid = _floor()
    for k, n in enumerate((1, 64, 65, 100)):
        solid[10 + 7 * k, 5:5 + n, 20] = True
    solid[40, 3:128, 40] = True   # 125 voxels up to the top of the world
    solid[41, 60:63, 40] = True   # ... with a stub: two nodes of different lengths in neighbouring lanes
    colour = _colours(solid)
    ctx = uploaded(solid, colour)
    pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, label="pillars")
    assert pieces["piece"]["voxels"].tolist() == [1, 64, 65, 100, 128] and summary["storedVoxels"] == 1 + 64 + 65 + 100 + 2 * 125
    _copy(ctx, solid, colour, ((0, 5, 0), (64, 70, 64)), 0, label="pillars cut at y0 and y1: nodes of 1, 64, 65, 65, 65 + 3")
    _copy(ctx, solid, colour, ((0, 6, 0), (64, 69, 64)), 0, label="pillars cut to 63")


def _lattice():
    """300 single voxels two apart, every one a colour of its own."""
    solid = _floor()
    for k in range(300):
        solid[2 + 2 * (k % 10), 4 + 2 * ((k // 10) % 6), 2 + 2 * (k // 60)] = True
    return solid, _colours(solid)


def test_many_single_voxel_pieces(uploaded):
    """The 64 nodes of a wave are 64 pieces, and there is more than one block of nodes."""
    solid, colour = _lattice()
    ctx = uploaded(solid, colour)
    pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, label="lattice")
    assert summary["floatingPieces"] == 300 == summary["storedPieces"] == summary["storedVoxels"] == summary["neededVoxels"]
    assert pieces["offset"].tolist() == list(range(300)) and (pieces["sum"] == 0).all() and (pieces["moment"] == 0).all()
    _, _, argb, mask = _host_call(ctx, WHOLE, GROUND, COPY, 8192, 300)
    assert len(set(argb[:300].tolist())) == 300 and mask[:300].all()
    assert [int(argb[k]) for k in (0, 1, 299)] == [int(colour[tuple(pieces[k]["piece"]["seed"])]) for k in (0, 1, 299)]
    _copy(ctx, solid, colour, WHOLE, 0, label="lattice and floor: 301 pieces, the floor the first")
    _copy(ctx, solid, colour, WHOLE, LARGEST, label="lattice, the floor anchored as the largest")


def test_two_nodes_of_one_column_joined_through_its_neighbour(uploaded):
    solid = _floor()
    solid[30, 10:15, 30] = True
    solid[30, 20:25, 30] = True
    solid[31, 10:25, 30] = True
    solid[29, 22:24, 30] = True
    colour = _colours(solid)
    ctx = uploaded(solid, colour)
    pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, label="two nodes in one column")
    assert summary["floatingPieces"] == 1 and int(pieces[0]["piece"]["voxels"]) == 27 and pieces[0]["piece"]["seed"].tolist() == [29, 23, 30]
    _copy(ctx, solid, colour, ((30, 0, 30), (32, 128, 31)), GROUND, label="without the stub: the seed is the upper node")
    _copy(ctx, solid, colour, ((30, 12, 30), (32, 22, 31)), OUTSIDE, voxel_capacity=500, label="cut at both ends: anchored through the voxels outside")


def test_capacity_edges(uploaded):
    solid, colour = interlocked(DIMS)
    for k, n in enumerate((1, 64, 65)):
        solid[40 + 3 * k, 5:5 + n, 50] = True
    solid[50:53, 30:32, 5:9] = True
    colour = _colours(solid)
    ctx = uploaded(solid, colour)
    every = liftmodel.lift(solid, colour, *WHOLE, GROUND, 8192, 1 << 62)
    volumes = [liftmodel.volume(p) for p in every.pieces["piece"]]
    m = len(volumes)
    assert m == 6 and volumes == [360, 288, 1, 64, 65, 24]
    # capacities 0: a REPORT that also sizes the pools
    pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, capacity=0, voxel_capacity=0, label="capacities 0")
    report, report_summary, _ = ctx.world_pieces(*WHOLE, GROUND, gpu.PIECES_REPORT)
    assert len(pieces) == 0 and summary["neededVoxels"] == sum(volumes) and summary["storedPieces"] == 0
    assert {k: summary[k] for k in report_summary} == report_summary
    listed, _, _ = _copy(ctx, solid, colour, WHOLE, GROUND, voxel_capacity=0, label="a list and no pool")
    assert listed["piece"].tobytes() == report.tobytes() and (listed["offset"] == -1).all() and listed["sum"].any()
    for k in range(1, m + 1):
        fits = sum(volumes[:k])
        pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, voxel_capacity=fits, label=f"room for exactly {k}", device=k == 2)
        assert summary["storedPieces"] == k and summary["storedVoxels"] == fits and (pieces["offset"][:k] >= 0).all() and (pieces["offset"][k:] == -1).all()
        pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, voxel_capacity=fits - 1, label=f"one short of {k}", device=k == 2)
        assert summary["storedPieces"] == k - 1 and int(pieces[k - 1]["offset"]) == -1 and summary["storedVoxels"] == fits - volumes[k - 1]
        assert summary["neededVoxels"] == sum(volumes)
    # room for the third piece but not for the second: a prefix, not a selection
    pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, voxel_capacity=361, label="room for 1 and 3")
    assert pieces["offset"].tolist() == [0, -1, -1, -1, -1, -1]
    for capacity in (0, 1, m - 1):
        pieces, summary, _ = _copy(ctx, solid, colour, WHOLE, GROUND, capacity=capacity, voxel_capacity=sum(volumes), label=f"pieceCapacity {capacity}")
        assert len(pieces) == capacity == summary["storedPieces"] and summary["floatingPieces"] == m and summary["neededVoxels"] == sum(volumes)
    # one pool alone
    want = liftmodel.lift(solid, colour, *WHOLE, GROUND, 8192, sum(volumes))
    _, _, argb, none, _ = ctx.world_lift_pieces(*WHOLE, GROUND, COPY, 5, 8192, sum(volumes), want_solid=False)
    _, _, none_too, mask, _ = ctx.world_lift_pieces(*WHOLE, GROUND, COPY, 5, 8192, sum(volumes), want_argb=False)
    assert none is None and none_too is None and argb.tobytes() == want.argb.tobytes() and mask.tobytes() == want.solid.tobytes()


# ---- REMOVE ------------------------------------------------------------------------------------------------------------------------------------------

def _debris():
    """Six pieces over a floor with a tower: the interlocked pair, three pillars, a slab.  -> (solid, colour)"""
    solid, _ = interlocked(DIMS)
    solid[3:6, 1:40, 3:6] = True  # a tower on the floor: anchored
    for k, n in enumerate((1, 64, 65)):
        solid[40 + 3 * k, 5:5 + n, 50] = True
    solid[50:53, 30:32, 5:9] = True
    return solid, _colours(solid)


def test_a_partial_remove_takes_the_stored_pieces_only(uploaded):
    solid, colour = _debris()
    ctx = uploaded(solid, colour)
    ws_before = _world_of(solid, colour)
    every = liftmodel.lift(solid, colour, *WHOLE, GROUND, 8192, 1 << 62)
    volumes = [liftmodel.volume(p) for p in every.pieces["piece"]]
    room = sum(volumes[:3]) + 10  # the frame, the bar and the first pillar; the 64-voxel pillar does not fit
    want = liftmodel.lift(solid, colour, *WHOLE, GROUND, 8192, room)
    assert want.summary["storedPieces"] == 3 and want.summary["floatingPieces"] == 6
    ws_after = _world_of(*want.removed)
    try:
        got = _host_call(ctx, WHOLE, GROUND, REMOVE, 8192, room)
        _assert_equals_model(got, want, room, "partial REMOVE")
        _assert_levels(ctx, ws_after, ws_before, 5, "without the three stored pieces")
        _check_world(ctx, ws_after, _frames(ws_after)[:2], "without the three stored pieces")
        solid_b, colour_b = want.removed
        assert solid_b[43, 5:69, 50].all() and not solid_b[11, 13, 4] and not solid_b[40, 5, 50]
        # a second call lifts the rest, through device pools and with a partial refresh of the levels
        rest = liftmodel.lift(solid_b, colour_b, *WHOLE, GROUND, 8192, 1000)
        assert rest.summary["storedPieces"] == 3 == rest.summary["floatingPieces"]
        pieces, summary, argb, mask = _device_call(ctx, WHOLE, GROUND, REMOVE, 8192, 1000, level_count=2)
        _assert_equals_model((pieces, summary, argb.cpu().numpy().view(np.uint32), mask.cpu().numpy()), rest, 1000, "the rest")
        ws_rest = _world_of(*rest.removed)
        try:
            _assert_levels(ctx, ws_rest, ws_after, 2, "the rest removed with levelCount 2")
            none, summary, _ = ctx.world_pieces(*WHOLE, GROUND, gpu.PIECES_REPORT)
            assert len(none) == 0 and summary["floatingPieces"] == 0 and summary["anchoredPieces"] == 1
            # nothing floats: a REMOVE with room changes nothing
            pieces, summary, _, _ = _host_call(ctx, WHOLE, GROUND, REMOVE, 8192, 1000)
            assert len(pieces) == 0 and summary["storedPieces"] == 0 == summary["neededVoxels"]
            _assert_levels(ctx, ws_rest, ws_after, 2, "after a REMOVE with nothing to remove")
        finally:
            ws_rest.close()
    finally:
        ws_before.close()
        ws_after.close()


def test_a_remove_without_room_changes_nothing(uploaded):
    solid, colour = _debris()
    ctx = uploaded(solid, colour)
    ws = _world_of(solid, colour)
    try:
        want = liftmodel.lift(solid, colour, *WHOLE, GROUND, 8192, 359)
        _assert_equals_model(_host_call(ctx, WHOLE, GROUND, REMOVE, 8192, 359), want, 359, "REMOVE one short of the first piece")
        want = liftmodel.lift(solid, colour, *WHOLE, GROUND, 0, 5000)
        _assert_equals_model(_host_call(ctx, WHOLE, GROUND, REMOVE, 0, 5000), want, 5000, "REMOVE with no list")
        assert want.summary["storedPieces"] == 0 and want.summary["neededVoxels"] == 802
        _assert_levels(ctx, ws, ws, 5, "after the two calls")
    finally:
        ws.close()


def test_round_trip_through_place_models(uploaded):
    """REMOVE with ample device pools, then every piece put back from those pools with cvx_world_place_models_device: the identity map at
    piece.min, FILL.  The world is the original again, voxel by voxel and level by level."""
    solid, colour = _lattice()
    solid[8:20, 50:52, 14:17] = True   # a U-frame and a bar above the lattice (which fills y 4 .. 14), as in interlocked()
    solid[8:10, 52:60, 14:17] = True
    solid[18:20, 52:60, 14:17] = True
    solid[11:17, 53:55, 4:28] = True
    colour = _colours(solid)
    ctx = uploaded(solid, colour)
    ws = _world_of(solid, colour)
    try:
        before_argb, before_solid = ctx.read_voxels(*WHOLE)
        assert before_solid.tobytes() == solid.transpose(0, 2, 1).astype(np.uint8).tobytes()
        want = liftmodel.lift(solid, colour, *WHOLE, GROUND, 8192, 2000)
        assert want.summary["storedPieces"] == 302 == want.summary["floatingPieces"]
        pieces, summary, argb, mask = _device_call(ctx, WHOLE, GROUND, REMOVE, 8192, 2000)
        _assert_equals_model((pieces, summary, argb.cpu().numpy().view(np.uint32), mask.cpu().numpy()), want, 2000, "REMOVE of 302 pieces")
        _, gone = ctx.read_voxels(*WHOLE, want_argb=False)
        assert int(gone.sum()) == DIMS[0] * DIMS[2], "the floor alone is left"
        for at in range(0, len(pieces), gpu.MODELS_MAX_MODELS):
            models, instances = [], []
            for k in range(at, min(at + gpu.MODELS_MAX_MODELS, len(pieces))):
                models.append(gpu.lifted_model(pieces, k, argb.data_ptr(), mask.data_ptr()))
                mn = pieces[k]["piece"]["min"]
                forward = [[1, 0, 0, int(mn[0])], [0, 1, 0, int(mn[1])], [0, 0, 1, int(mn[2])]]
                instances.append(gpu.model_instance(forward, models[-1][0], model=k - at, op=gpu.BRUSH_FILL))
            ctx.place_models_device(models, instances)
        after_argb, after_solid = ctx.read_voxels(*WHOLE)
        assert after_solid.tobytes() == before_solid.tobytes() and after_argb.tobytes() == before_argb.tobytes()
        _assert_levels(ctx, ws, ws, 5, "after the round trip")
    finally:
        ws.close()


# ---- rejected calls ----------------------------------------------------------------------------------------------------------------------------------

def test_rejected_calls_leave_the_world_alone(uploaded):
    solid, colour = _debris()
    ctx = uploaded(solid, colour)
    ws = _world_of(solid, colour)
    try:
        ok = dict(box_min=(0, 0, 0), box_max=DIMS, anchors=GROUND, op=REMOVE, capacity=16, voxel_capacity=5000)
        bad = [(dict(op=2), "bad op 2"), (dict(op=-1), "bad op -1"), (dict(voxel_capacity=-1), "voxelCapacity -1 is negative"),
               (dict(capacity=-1), "pieceCapacity"), (dict(want_argb=False, want_solid=False), "with no pool"),
               (dict(box_max=(0, 8, 8)), "empty"), (dict(box_min=(64, 0, 0), box_max=(70, 8, 8)), "outside the world"), (dict(anchors=8), "anchors"),
               (dict(level_count=6), "levelCount")]
        for change, match in bad:
            with pytest.raises(gpu.CvxError, match=match):
                ctx.world_lift_pieces(**{**ok, **change})
        with pytest.raises(gpu.CvxError, match="with no pool"):
            ctx.world_lift_pieces_device((0, 0, 0), DIMS, GROUND, None, None, REMOVE, voxel_capacity=10)
        _assert_levels(ctx, ws, ws, 5, "after the rejected calls")
        pieces, summary, _, _, _ = ctx.world_lift_pieces((0, 0, 0), DIMS, GROUND, COPY, voxel_capacity=5000)
        assert summary["floatingPieces"] == 6 == summary["storedPieces"]
        _assert_levels(ctx, ws, ws, 5, "after a COPY")
    finally:
        ws.close()
