"""GPU: cvx_world_lift_pieces and cvx_world_snapshot / _restore / _diff at the shapes compiled into their kernels.

The continuation of tests/test_gpu_world_kernel_limits_later.py for the two newest calls.  What is device-only in them (the host builds of
tests/lift_rules.cpp and tests/snapshot_rules.cpp cannot reach it):
  lift      lift_moments_kernel reduces nine 64-bit sums across a wave whose ACTIVE nodes share one root and lets the first active lane -- not lane
            0 -- add them; otherwise every active lane adds its own with 64-bit atomics.  Inactive lanes (anchored, or floating and not listed)
            take part with zeros.  lift_write_kernel scans the 64 node lengths of a wave, 0 for a node that is not stored, and finds the owner of
            every output voxel by a six-step search of the prefix sums.
  snapshot  snapshot_diff_count_kernel reduces 256 columns per workgroup (shuffles, then four wave partials through LDS) into one partial;
            snapshot_diff_reduce_kernel, ONE workgroup, walks the partials 256 at a time; the changed flags are scanned in chunks of 4096 into
            list positions.

Every case builds its volume in numpy (tests/limitworlds.py), asserts FROM THE VOLUME OR THE MODEL, before the device is called, that the wave
shape, length list or count it is named after is exactly that (tests/test_limit_worlds_cpu.py asserts the same without a device), and only then
compares the device's bytes and integers with the dense models (liftmodel, piecesmodel, snapshotmodel).  After a REMOVE or a restore every level
is compared: with the host-built LOD chain of the model's world, or with the bytes read before the edit.  No comparison has a tolerance.  One
fresh context per case."""
import numpy as np
import pytest
import torch

import liftmodel
import limitworlds as LW
import piecesmodel
import snapshotmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _box, _dense
from test_gpu_world_kernel_limits import _assert_world, _uploaded
from test_gpu_world_lift import REMOVE, _assert_equals_model, _colours, _copy, _host_call
from test_gpu_world_snapshot import IGNORE, assert_levels, cut, held, levels, regions, voxels
from test_world_pieces_cpu import OUTSIDE

pytestmark = pytest.mark.gpu

BOX = LW.PIECES_BOX
CARVE, PAINT = gpu.BRUSH_CARVE, gpu.BRUSH_PAINT
NOTHING = {"changedColumns": 0, "changedVoxels": 0, "min": (0, 0, 0), "max": (0, 0, 0)}


# ---- lift: the wave shapes of the moments kernel -------------------------------------------------------------------------------------------------------

def _remove_a_prefix(ctx, solid, colour, box, anchors, label):
    """One REMOVE whose voxelCapacity is one element short of the second half of the list: the first half is stored and removed.  The pools and
    the list against the model, every level against the model's world, and a REPORT that finds exactly the unstored pieces still floating."""
    every = liftmodel.lift(solid, colour, *box, anchors, 8192, 1 << 62)
    volumes = [liftmodel.volume(p) for p in every.pieces["piece"]]
    keep = len(volumes) // 2
    assert keep >= 1
    room = sum(volumes[:keep + 1]) - 1
    want = liftmodel.lift(solid, colour, *box, anchors, 8192, room)
    assert want.summary["storedPieces"] == keep < want.summary["floatingPieces"] == len(volumes), f"{label}: a proper prefix"
    _assert_equals_model(_host_call(ctx, box, anchors, REMOVE, 8192, room), want, room, f"{label}: REMOVE of {keep}")
    _assert_world(ctx, *want.removed, f"{label}: after the REMOVE of {keep}")
    left, summary, _ = ctx.world_pieces(*box, anchors, gpu.PIECES_REPORT, capacity=8192)
    assert left.tobytes() == every.pieces["piece"][keep:].tobytes() and summary["floatingPieces"] == len(volumes) - keep, f"{label}: the unstored pieces float on"
    assert piecesmodel.analyse(want.removed[0], *box, anchors)[0].tobytes() == left.tobytes()


def _moments_case(solid, copies, label):
    """COPY with exact voxelCapacity for every (pieceCapacity, the wave kinds asserted for it) of `copies`, on a fresh context over PIECES_BOX
    with no anchor bit; then _remove_a_prefix.  -> the (pieces, summary) of every COPY"""
    ranks = LW.node_ranks(solid, *BOX)
    for capacity, kinds in copies:
        got = LW.lift_wave_kinds(ranks, capacity)
        assert kinds(got), f"{label}, pieceCapacity {capacity}: the waves are {got}"
    colour = _colours(solid)
    ctx, ws = _uploaded(solid, colour)
    try:
        out = []
        for capacity, _ in copies:
            pieces, summary, _ = _copy(ctx, solid, colour, BOX, 0, capacity=capacity, label=f"{label}, pieceCapacity {capacity}")
            assert len(pieces) == min(capacity, summary["floatingPieces"]) == summary["storedPieces"]
            out.append((pieces, summary))
        _remove_a_prefix(ctx, solid, colour, BOX, 0, label)
        return out
    finally:
        ctx.close()
        ws.close()


@pytest.mark.parametrize("last", [64, 1, 63])
def test_lift_moments_where_every_wave_is_one_listed_piece(last):
    """Nine bars of one wave each, the last wave of 64, 1 and 63 nodes: every wave reduces once and its lane 0 adds."""
    solid = LW.pieces_bars(last=last)
    LW.assert_wave_shape("every wave one root" if last == 64 else f"last wave of {last}", LW.node_pieces(solid, *BOX))
    want = [("one root", 0, 64)] * 8 + [("one root", 0, last)]
    (pieces, _), = _moments_case(solid, [(8192, lambda kinds: kinds == want)], f"bars, the last of {last}")
    assert pieces["piece"]["voxels"].tolist() == [64] * 8 + [last] and pieces["sum"][0].tolist() == [0, 0, 63 * 64 // 2]


def test_lift_moments_where_every_node_is_its_own_piece():
    """2048 pieces of one node: every wave goes through the atomics, 64 addresses each.  pieceCapacity 0: nothing is listed, no moments are
    taken, and neededVoxels is still the model's."""
    solid = LW.pieces_checkerboard()
    LW.assert_wave_shape("every node its own root", LW.node_pieces(solid, *BOX))
    every = lambda kinds: kinds == [("atomics", None, 64)] * 32
    idle = lambda kinds: kinds == [("idle", None, 0)] * 32
    (_, none), (pieces, summary) = _moments_case(solid, [(0, idle), (8192, every)], "checkerboard")
    assert none["storedPieces"] == 0 and none["neededVoxels"] == 2048 == summary["neededVoxels"] == summary["storedVoxels"]
    assert not pieces["sum"].any() and not pieces["moment"].any()


def test_lift_moments_where_the_leader_is_not_lane_0():
    """The single-root path with lane 0 inactive.  A piece on lane 0 that comes LATER in the list than the piece behind it needs that piece's
    seed in an earlier wave (both orders are the column order), so pieces_lone_leader cannot give it (tests/test_limit_worlds_cpu.py asserts
    that); pieces_late_leader does: with pieceCapacity 5 wave 3 has lane 0 unlisted and lanes 1 .. 63 one listed piece, leader lane 1."""
    solid = LW.pieces_late_leader()
    floating, _, _ = piecesmodel.analyse(solid, *BOX, 0)
    ranks = LW.node_ranks(solid, *BOX)
    wave = LW.waves(ranks)[3]
    assert len(floating) == 12 and wave[0] == 5 and set(wave[1:].tolist()) == {4} and floating[4]["voxels"] == 64 and floating[5]["voxels"] == 1
    late = lambda kinds: kinds[3] == ("one root", 1, 63) and kinds[4:] == [("idle", None, 0)] * 4 and kinds[:3] == [("atomics", None, 64)] * 3
    first = lambda kinds: kinds[1] == ("one root", 1, 63) and kinds[0] == ("atomics", None, 64)
    full = lambda kinds: kinds == [("atomics", None, 64)] * 8
    (pieces, summary), _, _ = _moments_case(solid, [(5, late), (2, first), (8192, full)], "late leader")
    assert pieces[4]["sum"].tolist() == [0, 0, 63 * 64 // 2] and pieces[4]["moment"][2] == 63 * 64 * 127 // 6 and summary["floatingPieces"] == 12


def test_lift_moments_where_lane_0_alone_is_listed():
    """The mirror: lane 0's piece is listed and the bar on lanes 1 .. 63 is not.  One active lane, the wave is uniform and lane 0 leads."""
    solid = LW.pieces_lone_leader()
    LW.assert_wave_shape("lane 0 alone", LW.node_pieces(solid, *BOX))
    mirror = lambda kinds: kinds == [("atomics", None, 64)] * 2 + [("one root", 0, 1)] + [("idle", None, 0)] * 3
    full = lambda kinds: kinds == [("atomics", None, 64)] * 6
    (pieces, _), _ = _moments_case(solid, [(5, mirror), (8192, full)], "lone leader")
    assert pieces["piece"]["voxels"].tolist() == [1, 63, 1, 63, 1]


def test_lift_moments_with_two_listed_roots_and_unlisted_nodes_between():
    """Wave 1 is a, b, lone, a, b, lone, ...: with pieceCapacity 2 its 43 active lanes hold two roots and the 21 lanes between them are unlisted --
    the atomics path with inactive lanes."""
    solid = LW.pieces_two_roots_apart()
    ranks = LW.node_ranks(solid, *BOX)
    assert LW.waves(ranks)[1][:6].tolist() == [0, 1, 2, 0, 1, 3] and LW.piece_count(solid, *BOX) == 23
    two = lambda kinds: kinds == [("one root", 0, 64), ("atomics", None, 43), ("one root", 0, 64)]
    one = lambda kinds: kinds == [("one root", 0, 64), ("one root", 0, 22), ("idle", None, 0)]  # one active root, unlisted nodes between its lanes
    full = lambda kinds: kinds == [("one root", 0, 64), ("atomics", None, 64), ("one root", 0, 64)]
    (pieces, _), _, _ = _moments_case(solid, [(2, two), (1, one), (8192, full)], "two roots apart")
    assert pieces["piece"]["voxels"].tolist() == [64 + 22, 64 + 21]


def test_lift_around_256_listed_pieces():
    """pieceCapacity 255 / 256 / 257 over 257 floating pieces: the list head that travels with the totals, and the moments of exactly those."""
    solid = LW.pieces_checkerboard(257)
    LW.assert_wave_shape("257 listed", LW.node_pieces(solid, *BOX))
    active = lambda count: lambda kinds: [k[2] for k in kinds] == [64, 64, 64, min(count - 192, 64), max(count - 256, 0)]
    results = _moments_case(solid, [(255, active(255)), (256, active(256)), (257, active(257))], "257 pieces")
    assert [len(pieces) for pieces, _ in results] == [255, 256, 257]


# ---- lift: sums above 2^32 ------------------------------------------------------------------------------------------------------------------------------------

def test_lift_sums_above_32_bits():
    """Walls of 2400 voxels in 32 x 4096 x 32: wave 0 is the 64 nodes of one piece (the reduction carries node sums of 4.6e9 to a total of 2.9e11),
    wave 1 alternates between two combs (the 64-bit atomics with operands above 2^32).  Also lift_write_kernel with 64 long nodes in a wave."""
    solid, box = LW.lift_tall_world(), LW.LIFT_TALL_BOX
    ranks, lengths = LW.node_ranks(solid, *box), LW.node_lengths(solid, *box)
    assert LW.lift_wave_kinds(ranks, 8192) == [("one root", 0, 64), ("atomics", None, 64)] and LW.waves(ranks)[1].tolist() == [1, 2] * 32
    assert lengths[:64].tolist() == [LW.LIFT_TALL_WALL] * 64 and LW.pillar_moment(LW.LIFT_TALL_WALL) > 1 << 32
    assert sorted(set(lengths[64:].tolist())) == [1, 2400, 2406]
    colour = LW.unique_colours(solid)
    want = liftmodel.lift(solid, colour, *box, 0, 8192, 1 << 62)
    assert len(want.pieces) == 3 and all(max(int(v) for v in p["moment"]) > 1 << 32 for p in want.pieces), "every listed piece has a sum above 2^32"
    wall = want.pieces[0]
    assert int(wall["moment"][1]) == 64 * LW.pillar_moment(LW.LIFT_TALL_WALL) and int(wall["sum"][1]) == 64 * (2399 * 2400 // 2), "the model's integers are exact"
    ctx, ws = _uploaded(solid, colour)
    try:
        pieces, summary, _ = _copy(ctx, solid, colour, box, 0, label="tall walls")
        assert summary["storedPieces"] == 3 and summary["storedVoxels"] == 64 * 2400 + 32 * 2406 + 32 * 2400
        assert LW.lift_wave_kinds(ranks, 2)[1] == ("one root", 0, 32), "the third piece unlisted: one active root with unlisted nodes between its lanes"
        _copy(ctx, solid, colour, box, 0, capacity=2, label="tall walls, the third piece unlisted")
        _remove_a_prefix(ctx, solid, colour, box, 0, "tall walls")
    finally:
        ctx.close()
        ws.close()


# ---- lift: the write kernel's scan and search -----------------------------------------------------------------------------------------------------------------------

def _lengths_case(pattern, label, voxel_capacity=None, stored=None):
    """COPY of LW.lift_lengths(pattern) on a fresh context, every voxel a colour of its own: the per-wave length lists asserted from the volume,
    then the pools whole against the model (_copy: the sentinel behind storedVoxels untouched, twice on the host, once through _device)."""
    solid, box = LW.lift_lengths(pattern), LW.LIFT_LENGTH_BOX
    expected = list(pattern) if stored is None else stored
    scanned = LW.stored_lengths(solid, *box, OUTSIDE, 8192, (1 << 62) if voxel_capacity is None else voxel_capacity)
    assert [w.tolist() for w in LW.waves(scanned)] == LW.waves(expected), f"{label}: the write kernel scans {scanned.tolist()}"
    colour = _colours(solid)
    ctx, ws = _uploaded(solid, colour)
    try:
        pieces, summary, want = _copy(ctx, solid, colour, box, OUTSIDE, voxel_capacity=voxel_capacity, label=label)
        assert summary["storedVoxels"] == sum(expected) and summary["storedPieces"] == sum(1 for v in expected if v)
        assert summary["floatingPieces"] == sum(1 for v in pattern if v) and summary["anchoredPieces"] == sum(1 for v in pattern if not v)
        assert len(set(want.argb.tolist())) == sum(expected), "every stored voxel has a colour of its own"
        return pieces, summary
    finally:
        ctx.close()
        ws.close()


@pytest.mark.parametrize("name", sorted(LW.LIFT_LENGTH_PATTERNS))
def test_lift_write_with_the_node_lengths(name):
    """Zero-length lanes (nodes of anchored pillars) at chosen places of the wave, and wave totals on both sides of the 64 voxels of a step."""
    pattern, totals = LW.LIFT_LENGTH_PATTERNS[name]
    if totals is not None:
        assert [sum(w) for w in LW.waves(pattern)] == totals
    _lengths_case(pattern, name)


def test_lift_write_behind_a_prefix_that_stores_fewer_pieces_than_are_listed():
    """100 pillars of five voxels and room for 70 and four voxels more: the nodes of the 30 listed and unstored pieces add to the moments and have
    length 0 in the write -- wave 1 has six stored lanes, 30 zeros and 28 lanes behind the nodes."""
    pieces, _ = _lengths_case([5] * 100, "room for 70 of 100", voxel_capacity=5 * 70 + 4, stored=[5] * 70 + [0] * 30)
    assert (pieces["offset"][:70] == 5 * np.arange(70)).all() and (pieces["offset"][70:] == -1).all()
    assert (pieces["sum"][:, 1] == 10).all() and (pieces["moment"][:, 1] == 30).all(), "listed and not stored: the sums are taken all the same"


# ---- snapshot: above 256 workgroups --------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def terrain():
    """The 256 x 32 x 512 terrain, built once: (the volume as (X, Z, Y) arrays, as cvx_world_read_voxels gives it; the host-built world)."""
    from test_world_light_cpu import model_world

    solid = LW.snap_terrain()
    colour = _dense(solid)
    ws = model_world(LW.SNAP_DIMS, solid, colour)
    yield (np.ascontiguousarray(solid.transpose(0, 2, 1)), np.ascontiguousarray(colour.transpose(0, 2, 1))), ws
    ws.close()


def _edited(before, strokes):
    """Box strokes (CARVE, PAINT) on (X, Z, Y) arrays -> the volume after them."""
    solid, argb = before[0].copy(), before[1].copy()
    for s in strokes:
        (x0, y0, z0), (x1, y1, z1) = s["a"], s["b"]
        where = (slice(x0, x1), slice(z0, z1), slice(y0, y1))
        if s["op"] == CARVE:
            solid[where], argb[where] = False, 0
        else:
            assert s["op"] == PAINT
            argb[where] = np.where(solid[where], np.uint32(s["argb"]), 0)
    return solid, argb


def _voxel(op, x, y, z, argb=0):
    return _box(op, (x, y, z), (x + 1, y + 1, z + 1), argb)


def _snapshot_case(ctx, before, rect, strokes, label, lists=True):
    """Snapshot at levelCount 0, the strokes at levelCount 0, then the diff with both flags against the model of (before, before + strokes) at the
    capacities 0, 1, changed - 1, changed, changed + 1 and through the _device variant; then the restore: the held level, every whole level and
    an empty diff.  -> {flags: the model's summary}"""
    base = levels(ctx)
    after = _edited(before, strokes)
    out = {}
    with ctx.world_snapshot(*rect, 0) as snapshot:
        assert held(snapshot) == tuple(rect)
        taken = regions(ctx, rect, 0)
        ctx.brush(strokes, 0)
        now = voxels(ctx, LW.SNAP_DIMS)
        assert (now[0] == after[0]).all() and (now[1] == after[1]).all(), f"{label}: the strokes did what the test's model of them does"
        for flags in (0, IGNORE):
            want, want_summary = snapshotmodel.diff(cut(before, rect), cut(after, rect), rect[:2], flags)
            changed = len(want)
            for capacity in sorted({0, 1, max(changed - 1, 0), changed, changed + 1}) if lists else [changed + 1]:
                got, summary = snapshot.diff(flags, capacity=capacity)
                assert summary == want_summary, f"{label}, flags {flags}, capacity {capacity}: {summary} != {want_summary}"
                assert got.tobytes() == want[:capacity].tobytes(), f"{label}, flags {flags}: the list of capacity {capacity} differs"
            buffer = torch.full((changed + 2, 4), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert snapshot.diff_device(buffer.data_ptr(), changed + 1, flags) == want_summary, f"{label}, flags {flags}: _device"
            torch.cuda.synchronize()
            back = buffer.cpu().numpy()
            assert back[:changed].tobytes() == want.tobytes() and (back[changed:] == -7).all(), f"{label}, flags {flags}: the device list"
            out[flags] = want_summary
        snapshot.restore()
        assert_levels(regions(ctx, rect, 0), taken, f"{label}: restored, the rectangle")
        assert_levels(levels(ctx), base, f"{label}: restored, every whole level")
        changes, summary = snapshot.diff()
        assert len(changes) == 0 and summary == NOTHING, f"{label}: a diff behind the restore"
    return out


@pytest.mark.parametrize("pattern", ["scattered", "every column"])
@pytest.mark.parametrize("name", sorted(LW.SNAP_RECTS))
def test_snapshot_diff_above_256_workgroups(terrain, name, pattern):
    """Rectangles of 256, 257 (full and partial) and 512 count workgroups: the reduce kernel's threads combine a second partial, and list positions
    cross the scan's chunks.  scattered: the first and the last column of every chunk and one column in an even and an odd workgroup of it, a
    one-voxel CARVE or PAINT each.  every column: a carve through the whole rectangle."""
    before, ws = terrain
    rect, facts = LW.SNAP_RECTS[name]
    n, groups, last, chunks = LW.snap_counts(rect)
    assert (n, groups, last) == facts and groups >= 256 and chunks >= 16
    x0, z0, sx, sz = rect
    if pattern == "scattered":
        indices = LW.snap_scattered(rect)
        places = [LW.snap_place(rect, i) for i in indices]
        for c in range(chunks):
            mine = [p for i, p in zip(indices, places) if i // LW.SNAP_CHUNK == c]
            assert len(mine) >= 2 and (c == chunks - 1 and n % LW.SNAP_CHUNK != 0 or {p[1] % 2 for p in mine} == {0, 1}), f"chunk {c}: {mine}"
        assert indices[-1] == n - 1 and any(p[1] >= 256 for p in places) == (groups > 256)
        strokes = [_voxel(PAINT, x, 1, z, 0xFF000000 | k) if k % 3 == 0 else _voxel(CARVE, x, 2 + k % 3, z) for k, ((x, z), _, _, _) in enumerate(places)]
        changed = (len(indices), len(indices) - len(indices[::3]))
    else:
        strokes = [_box(CARVE, (x0, 2, z0), (x0 + sx, 4, z0 + sz))]
        changed = (n, n)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        summaries = _snapshot_case(ctx, before, rect, strokes, f"{name}, {pattern}")
        assert (summaries[0]["changedColumns"], summaries[IGNORE]["changedColumns"]) == changed
    finally:
        ctx.close()


def test_snapshot_of_the_whole_world_at_every_level(terrain):
    """levelCount 5 over 131 072 columns: captured, carved through, restored."""
    before, ws = terrain
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        base = levels(ctx)
        whole = LW.SNAP_RECTS["the whole world"][0]
        with ctx.world_snapshot(*whole, 5) as snapshot:
            taken = regions(ctx, whole, 5)
            ctx.brush([_box(CARVE, (0, 1, 0), (256, 9, 512)), _box(PAINT, (0, 0, 0), (256, 1, 512), 0xFF445566)], 5)
            assert all(a != b for a, b in zip(levels(ctx), base)), "every level changes"
            summary = snapshot.diff(capacity=0)[1]
            assert summary["changedColumns"] == 131072 and (summary["min"], summary["max"]) == ((0, 0, 0), (256, 9, 512))
            snapshot.restore()
            assert_levels(regions(ctx, whole, 5), taken, "the whole world restored, the held levels")
            assert_levels(levels(ctx), base, "the whole world restored")
    finally:
        ctx.close()


# ---- snapshot: where the one changed column lies ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", LW.SNAP_ONE_INDICES)
def test_snapshot_diff_of_one_changed_column(terrain, index):
    """One voxel painted, then one voxel carved, in the column at linear index `index` of the 255 x 258 rectangle: the first and the last lane of
    every wave of workgroup 0, the first lane of workgroup 1, both sides of the 256th workgroup's end, and the last column -- a lane of the
    partial workgroup 256, whose other lanes reduce the neutral partial."""
    before, ws = terrain
    rect = LW.SNAP_ONE_RECT
    (x, z), group, wave, lane = LW.snap_place(rect, index)
    assert (group * 256 + wave * 64 + lane) == index and before[0][x, z, :5].all()
    if index == 65789:
        assert (group, wave, lane) == (256, 3, 61) and (x, z) == (rect[0] + rect[2] - 1, rect[1] + rect[3] - 1) and LW.snap_counts(rect)[2] == 254
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        painted = _snapshot_case(ctx, before, rect, [_voxel(PAINT, x, 3, z, 0xFF0A0B0C)], f"index {index}, PAINT", lists=False)
        assert painted[0] == {"changedColumns": 1, "changedVoxels": 1, "min": (x, 3, z), "max": (x + 1, 4, z + 1)}
        assert painted[IGNORE] == NOTHING, "a colour alone is nothing under IGNORE_COLOUR"
        carved = _snapshot_case(ctx, before, rect, [_voxel(CARVE, x, 2, z)], f"index {index}, CARVE", lists=False)
        assert carved[0] == carved[IGNORE] == {"changedColumns": 1, "changedVoxels": 1, "min": (x, 2, z), "max": (x + 1, 3, z + 1)}
    finally:
        ctx.close()


def test_snapshot_diff_box_from_two_workgroups(terrain):
    """Two changed columns: min[0], max[1] and max[2] of the box come from workgroup 0, max[0], min[1] and min[2] from the partial workgroup 256."""
    before, ws = terrain
    rect = LW.SNAP_ONE_RECT
    (ia, ya), (ib, yb) = LW.snap_box_pair(rect)
    (xa, za), ga, _, _ = LW.snap_place(rect, ia)
    (xb, zb), gb, _, _ = LW.snap_place(rect, ib)
    assert (ga, gb) == (0, 256) and xa < xb and za > zb and ya > yb
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        got = _snapshot_case(ctx, before, rect, [_voxel(CARVE, xa, ya, za), _voxel(CARVE, xb, yb, zb)], "two columns")
        assert got[0] == got[IGNORE] == {"changedColumns": 2, "changedVoxels": 2, "min": (xa, yb, zb), "max": (xb + 1, ya + 1, za + 1)}
    finally:
        ctx.close()
