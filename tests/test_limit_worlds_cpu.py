"""CPU (no GPU needed): the worlds of tests/test_gpu_world_kernel_limits_later.py and tests/test_gpu_world_kernel_limits_newest.py are what their
names say.

Every count the GPU cases assert before they call the device -- tile totals, wave compositions, cell counts, piece and cavity counts, element and
word counts -- is asserted here from the numpy volumes alone (tests/limitworlds.py) and, where a dense model has a say (spreadmodel, navmodel,
piecesmodel, cavitymodel), against the model: a GPU case cannot rest on a world that lies on the other side of its limit."""
import numpy as np
import pytest

import cavitymodel
import limitworlds as LW
import navmodel
import piecesmodel
import spreadmodel

GROUND, OUTSIDE = piecesmodel.GROUND, piecesmodel.OUTSIDE
BOX = LW.PIECES_BOX


# ---- the air side ----------------------------------------------------------------------------------------------------------------------------------------

def test_the_complement_of_the_bars_has_the_same_nodes():
    bars = LW.pieces_bars()
    rock = LW.complement(bars)
    assert (LW.air_tops(rock, *BOX) == LW.run_tops(bars, *BOX)).all() and len(LW.air_tops(rock, *BOX)) == 576
    assert (LW.node_cavities(rock, *BOX) == LW.node_pieces(bars, *BOX)).all()
    cavities, summary, _ = cavitymodel.analyse(rock, *BOX, 0, 0)
    assert summary["enclosedCavities"] == 9 and summary["enclosedVoxels"] == 576 and summary["openRegions"] == 0 and len(cavities) == 9


@pytest.mark.parametrize("name", sorted(LW.WAVE_SHAPES))
def test_wave_shapes_of_both_rules(name):
    build, count, some = LW.WAVE_SHAPES[name]
    solid = build()
    rock = LW.complement(solid)
    LW.assert_wave_shape(name, LW.node_pieces(solid, *BOX))
    LW.assert_wave_shape(name, LW.node_cavities(rock, *BOX))
    assert LW.piece_count(solid, *BOX) == count == LW.cavity_count(rock, *BOX)
    assert rock[:, 63, :].all() and rock[:, 0, :].all(), "the box lies inside rock: no sky node"
    _, summary, _ = cavitymodel.analyse(rock, *BOX, 0, 0)
    assert summary["enclosedCavities"] == summary["selectedCavities"] == count and summary["openRegions"] == 0
    _, summary, _ = cavitymodel.analyse(rock, *BOX, 0, some)
    assert 0 < summary["selectedCavities"] < count, "the voxel limit selects some cavities, not all"


# ---- one node with a bit --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lane", LW.BITS_LANES)
@pytest.mark.parametrize("anchor", [OUTSIDE, GROUND])
def test_one_node_anchors_its_piece(anchor, lane):
    solid, box, column = LW.bars_one_node_down(lane, to_ground=anchor == GROUND)
    LW.assert_one_node_in_its_wave(LW.run_tops(solid, *box), LW.node_pieces(solid, *box), column, lane)
    pieces, summary, _ = piecesmodel.analyse(solid, *box, anchor)
    assert summary["anchoredPieces"] == 1 and summary["floatingPieces"] == 8 and 2 * LW.BITS_ROW not in pieces["min"][:, 0].tolist()
    plain = solid.copy()
    plain[column[0], :10 + LW.BITS_ROW % 3, column[1]] = False  # without the node's extension nothing is anchored: no other node has the bit
    if anchor == OUTSIDE:
        plain[:, 0, :] = True
    assert piecesmodel.analyse(plain, *box, anchor)[1]["anchoredPieces"] == 0


@pytest.mark.parametrize("lane", LW.BITS_LANES)
def test_one_node_opens_its_cavity(lane):
    solid, column = LW.bars_one_node_open(lane)
    LW.assert_one_node_in_its_wave(LW.air_tops(solid, *BOX), LW.node_cavities(solid, *BOX), column, lane)
    cavities, summary, _ = cavitymodel.analyse(solid, *BOX, 0x08, 0)
    assert summary["openRegions"] == 1 and summary["enclosedCavities"] == 8 and 2 * LW.BITS_ROW not in cavities["min"][:, 0].tolist()
    assert cavitymodel.analyse(solid, *BOX, 0, 0)[1]["enclosedCavities"] == 9
    assert cavitymodel.analyse(LW.complement(LW.pieces_bars()), *BOX, 0x08, 0)[1]["openRegions"] == 0, "no other node reaches the +Y face"


# ---- the comb ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plate", [True, False])
def test_the_comb(plate):
    solid, bars = LW.comb(plate)
    rock = LW.complement(solid)
    tops = LW.run_tops(solid, *BOX)
    assert bars == 31 * 32 and LW.piece_count(solid, *BOX) == LW.cavity_count(rock, *BOX) == (1 if plate else bars)
    assert tops[0].tolist() == [0, 62, 0] and (LW.air_tops(rock, *BOX) == tops).all()
    along = (tops[:, 0] < 63).sum()
    assert along == 63 * bars == int(solid[:63, 1:, :].sum()), "every voxel along a bar is a node of its own"
    pieces, _, _ = piecesmodel.analyse(solid, *BOX, 0)
    roots = LW.node_pieces(solid, *BOX)
    if plate:
        assert pieces[0]["seed"].tolist() == [0, 62, 0] and int(pieces[0]["voxels"]) == int(solid[:, 1:, :].sum())
        assert not solid[:63, 1:, 1::2].any() and not solid[:63, 1::2, :].any(), "no contact between bars before the plate at the last x"
    else:
        assert len(pieces) == bars and (pieces["voxels"] == 64).all() and (pieces["seed"][:, 0] == 0).all(), "a bar's smallest node is the one at x = 0"
        assert len(set(roots)) == bars


# ---- spread --------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layers", [3, 32])
def test_the_sealed_corridor(layers):
    solid, cells = LW.spread_sealed_corridor(layers)
    count = LW.spread_corridor_facts(solid, cells)
    assert count == 35 * layers + layers - 1 and (layers != 32 or count == 1151)
    assert LW.spread_row_sweeps(layers) > LW.SPREAD_SWEEPS and (layers != 3 or LW.spread_row_sweeps(2) <= LW.SPREAD_SWEEPS), "3 layers: the shortest that needs a re-queue"
    whole = ((0, 0, 0), LW.SPREAD_DIMS)
    for seed, far in ((cells[0], cells[-1]), (cells[-1], cells[0])):
        field, summary = spreadmodel.field(solid, *whole, [seed], spreadmodel.AIR, 0x3F, 65534)
        assert summary["reached"] == summary["passable"] == count and summary["largestDistance"] == count - 1 == field[far[0], far[2], far[1]]
    cut = count // 2
    _, summary = spreadmodel.field(solid, *whole, [cells[0]], spreadmodel.AIR, 0x3F, cut)
    assert summary["reached"] == cut + 1 and summary["largestDistance"] == cut


def test_spread_boxes_around_the_workgroups():
    world = LW.spread_open_world()
    for n, (lo, hi) in LW.SPREAD_ELEMENT_BOXES.items():
        assert LW.spread_counts(lo, hi)[0] == n and not world[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].any(), n
        assert all(0 <= lo[a] < hi[a] <= LW.SPREAD_TALL[a] for a in range(3)), "inside the world: every voxel is open air"
    assert sorted(LW.SPREAD_ELEMENT_BOXES) == [2047, 2048, 4095, 4096, 4097]
    for words, (lo, hi) in LW.SPREAD_WORD_BOXES.items():
        assert LW.spread_counts(lo, hi)[1] == words, words
    assert sorted(LW.SPREAD_WORD_BOXES) == [63, 64, 65]


@pytest.mark.parametrize("parity", [0, 1])
def test_spread_seeds_that_share_a_word(parity):
    lo, hi, seeds, (a, b), index = LW.spread_shared_word(parity)
    assert (hi[1] - lo[1]) % 2 == 1 and index[1] == index[0] + 1 and index[0] % 2 == parity, "parity 0: one word; parity 1: two words"
    assert len(seeds) == 128 and [s[:3] for s in seeds[0::2]] == [a] * 64 and [s[:3] for s in seeds[1::2]] == [b] * 64
    for voxel_seeds in (seeds[0::2], seeds[1::2]):
        starts = [s[3] for s in voxel_seeds]
        assert len(set(starts)) == 64 and starts.index(min(starts)) == 31
    field, summary = spreadmodel.field(LW.spread_open_world(), lo, hi, seeds, spreadmodel.AIR, 0x33, 200)
    assert summary["seedsUsed"] == 128
    assert field[a[0] - lo[0], a[2] - lo[2], a[1] - lo[1]] == 3 and field[b[0] - lo[0], b[2] - lo[2], b[1] - lo[1]] == 40, "no vertical step: each voxel keeps its own smallest start"


# ---- nav -----------------------------------------------------------------------------------------------------------------------------------------------------

def assert_goals_cross_the_edge(solid, call, tile):
    """Ways ENTER the heavy tile (its slab nodes among them are nearer to the goal beyond its edge) and LEAVE it (nodes outside are nearer to the goal
    inside): with both goals in one build the tile needs its halo's distances, and its neighbours need its own."""
    entering, slab_nodes, leaving = LW.nav_goal_sides(solid, call, tile, LW.nav_limit_goals(call, tile))
    assert slab_nodes >= 1000 and entering > slab_nodes and leaving >= 500, (entering, slab_nodes, leaving)


@pytest.mark.parametrize("total", [1535, 1536, 1537])
@pytest.mark.parametrize("name", sorted(LW.NAV_LIMIT_CASES))
def test_nav_tile_totals_at_the_limit(name, total):
    tile, box_min = LW.NAV_LIMIT_CASES[name]
    solid, call, built = LW.nav_limit_world(total, tile, box_min)
    totals = LW.nav_tile_totals(solid, call)
    assert totals[tile] == total and max(v for t, v in totals.items() if t != tile) <= 18 * 18
    assert totals[(0, 0)] == (total if tile == (0, 0) else 17 * 17)
    _, summary = navmodel.analyse(solid, *LW.nav_tile_box(call, tile), *call[2:6], [(0, 0, 0)], 0)
    assert summary["nodes"] == total, "the model counts the same nodes over the tile and its halo"
    _, summary = navmodel.analyse(solid, *call[:6], LW.nav_limit_goals(call, tile), 0)
    assert summary["goalsResolved"] == 2 and summary["reached"] == summary["nodes"] == int(LW.nav_column_nodes(solid, call)[0].sum())
    assert_goals_cross_the_edge(solid, call, tile)


def test_nav_heavy_columns_on_a_tiles_last_column():
    solid, call, built = LW.nav_limit_world(1537, (2, 2), edge=14 * LW.NAV_SLABS, neighbour_total=1536)
    totals = LW.nav_tile_totals(solid, call)
    assert built == {(2, 2): 1537, (3, 2): 1536} and all(totals[t] == v for t, v in built.items())
    assert max(v for t, v in totals.items() if t not in built) <= 18 * 18
    assert solid[47, 2:63:2, 33:47].all() and not solid[48, 1:, :].any(), "the shared columns are the heavy tile's last, the neighbour's halo"
    assert_goals_cross_the_edge(solid, call, (2, 2))


def test_the_nav_tile_corridor():
    for slab_columns, side in ((0, "LDS"), (36, "global memory")):
        solid, call, cells = LW.nav_tile_corridor(slab_columns)
        c = np.array(cells)
        assert len(cells) == 135 == len(set(cells)) and (np.abs(np.diff(c, axis=0)).sum(axis=1) == 1).all()
        assert (c[:, 0] // 16 == 2).all() and (c[:, 2] // 16 == 2).all(), "inside one tile"
        totals = LW.nav_tile_totals(solid, call)
        assert (totals[LW.NAV_CORRIDOR_TILE] <= LW.NAV_TILE_NODES) == (side == "LDS"), totals[LW.NAV_CORRIDOR_TILE]
        assert max(v for t, v in totals.items() if t != LW.NAV_CORRIDOR_TILE) <= LW.NAV_TILE_NODES
        want, summary = navmodel.analyse(solid, *call[:6], [cells[0]], 0)
        assert summary["reached"] == 135 and summary["largestDistance"] == 134 == want[cells[-1]]["distance"]
        assert LW.nav_corridor_row_sweeps(solid, call, cells) == 120 > LW.NAV_SWEEPS
    assert totals[LW.NAV_CORRIDOR_TILE] == 324 + 135 + 36 * 30


# ---- lift: the waves of the moments kernel (tests/test_gpu_world_kernel_limits_newest.py) ---------------------------------------------------------------------

def test_lift_wave_kinds_of_the_pieces_worlds():
    """What lift_moments_kernel's waves hold in the worlds the pieces tests already use, for the pieceCapacity each GPU case passes."""
    for last in (64, 1, 63):
        ranks = LW.node_ranks(LW.pieces_bars(last=last), *BOX)
        assert LW.lift_wave_kinds(ranks, 8192) == [("one root", 0, 64)] * 8 + [("one root", 0, last)]
    ranks = LW.node_ranks(LW.pieces_checkerboard(), *BOX)
    assert ranks.tolist() == list(range(2048)), "a piece per node: the list order is the node order"
    assert LW.lift_wave_kinds(ranks, 8192) == [("atomics", None, 64)] * 32 and LW.lift_wave_kinds(ranks, 0) == [("idle", None, 0)] * 32
    ranks = LW.node_ranks(LW.pieces_checkerboard(257), *BOX)
    for capacity in (255, 256, 257):
        assert [k[2] for k in LW.lift_wave_kinds(ranks, capacity)] == [64, 64, 64, min(capacity - 192, 64), max(capacity - 256, 0)]


def test_the_lone_leader_always_comes_before_its_bar():
    """In pieces_lone_leader lane 0's piece precedes the bar of its wave in the list, in every wave: a prefix of the list can leave the bar out
    (the mirror case: lane 0 the only active lane) and never the lone voxel alone.  The node order and the list order are both the column order,
    so a piece on lane 0 can come later than the one behind it only when that one has a node in an earlier wave: pieces_late_leader."""
    solid = LW.pieces_lone_leader()
    ranks = LW.node_ranks(solid, *BOX)
    for r, w in enumerate(LW.waves(ranks)):
        assert w[0] == 2 * r and set(w[1:].tolist()) == {2 * r + 1}
    for capacity in range(13):
        for path, leader, active in LW.lift_wave_kinds(ranks, capacity):
            assert path == "idle" or (path == "one root" and (leader, active) == (0, 1)) or (path == "atomics" and active == 64)
    assert LW.lift_wave_kinds(ranks, 5) == [("atomics", None, 64)] * 2 + [("one root", 0, 1)] + [("idle", None, 0)] * 3


def test_the_late_leader():
    solid = LW.pieces_late_leader()
    floating, _, _ = piecesmodel.analyse(solid, *BOX, 0)
    assert floating["voxels"].tolist() == [63, 64, 1] * 4 and LW.node_count(solid, *BOX) == 8 * 64
    ranks = LW.node_ranks(solid, *BOX)
    for u in range(4):
        pad, bar, lone = 3 * u, 3 * u + 1, 3 * u + 2
        assert LW.waves(ranks)[2 * u].tolist() == [pad] * 63 + [bar] and LW.waves(ranks)[2 * u + 1].tolist() == [lone] + [bar] * 63
        kinds = LW.lift_wave_kinds(ranks, 3 * u + 2)  # pad and bar listed, the lone voxel not
        assert kinds[2 * u + 1] == ("one root", 1, 63) and kinds[2 * u] == ("atomics", None, 64) and kinds[2 * u + 2:] == [("idle", None, 0)] * (6 - 2 * u)
    assert LW.lift_wave_kinds(ranks, 8192) == [("atomics", None, 64)] * 8


def test_two_roots_apart():
    solid = LW.pieces_two_roots_apart()
    floating, _, _ = piecesmodel.analyse(solid, *BOX, 0)
    assert floating["voxels"].tolist() == [64 + 22, 64 + 21] + [1] * 21
    ranks = LW.node_ranks(solid, *BOX)
    wave = LW.waves(ranks)[1]
    assert (wave[0::3] == 0).all() and (wave[1::3] == 1).all() and (wave[2::3] >= 2).all() and len(set(wave[2::3].tolist())) == 21
    assert LW.lift_wave_kinds(ranks, 2) == [("one root", 0, 64), ("atomics", None, 43), ("one root", 0, 64)]
    assert LW.lift_wave_kinds(ranks, 1) == [("one root", 0, 64), ("one root", 0, 22), ("idle", None, 0)]


def test_the_tall_walls_have_sums_above_32_bits():
    """The model's integers against sums taken voxel by voxel in Python integers, and against the closed form of a pillar."""
    import liftmodel

    solid, box = LW.lift_tall_world(), LW.LIFT_TALL_BOX
    ranks, lengths = LW.node_ranks(solid, *box), LW.node_lengths(solid, *box)
    assert LW.lift_wave_kinds(ranks, 8192) == [("one root", 0, 64), ("atomics", None, 64)] and LW.waves(ranks)[1].tolist() == [1, 2] * 32
    assert LW.lift_wave_kinds(ranks, 2) == [("one root", 0, 64), ("one root", 0, 32)]
    assert lengths[:64].tolist() == [2400] * 64 and lengths[64:].tolist() == ([2406, 1, 1, 1, 1, 2400, 1, 1] * 8)
    assert LW.pillar_moment(2344) < 1 << 32 < LW.pillar_moment(2345) < LW.pillar_moment(2400)
    colour = LW.unique_colours(solid)
    assert len(np.unique(colour[solid])) == int(solid.sum())
    want = liftmodel.lift(solid, colour, *box, 0, 8192, 1 << 62)
    assert len(want.pieces) == 3 and want.pieces["sum"].dtype == np.uint64 and want.pieces["moment"].dtype == np.uint64
    for p in want.pieces:
        sums, moments = LW.brute_sums(solid, *box, p["piece"])
        assert [int(v) for v in p["sum"]] == sums and [int(v) for v in p["moment"]] == moments
        assert max(moments) > 1 << 32 and max(sums) < 1 << 32
    assert int(want.pieces[0]["moment"][1]) == 64 * LW.pillar_moment(2400) == 294727705600


# ---- lift: the lengths the write kernel scans ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(LW.LIFT_LENGTH_PATTERNS))
def test_lift_lengths(name):
    pattern, totals = LW.LIFT_LENGTH_PATTERNS[name]
    solid = LW.lift_lengths(pattern)
    box = LW.LIFT_LENGTH_BOX
    assert LW.node_count(solid, *box) == len(pattern) == LW.piece_count(solid, *box), "a node and a piece per entry"
    assert LW.stored_lengths(solid, *box, OUTSIDE, 8192, 1 << 62).tolist() == list(pattern)
    assert (LW.node_lengths(solid, *box) == np.where(np.array(pattern) > 0, pattern, 2)).all()
    _, summary, _ = piecesmodel.analyse(solid, *box, OUTSIDE)
    assert summary["anchoredPieces"] == pattern.count(0) and summary["floatingVoxels"] == sum(pattern)
    if totals is not None:
        assert [sum(w) for w in LW.waves(pattern)] == totals


def test_lift_length_patterns_cover_the_issue():
    P = {name: pattern for name, (pattern, _) in LW.LIFT_LENGTH_PATTERNS.items()}
    assert P["lane 0 zero"][0] == 0 and all(P["lane 0 zero"][1:]) and P["lane 63 zero"][63] == 0 and all(P["lane 63 zero"][:63])
    assert P["lanes 1 to 62 zero"][0] and P["lanes 1 to 62 zero"][63] and not any(P["lanes 1 to 62 zero"][1:63])
    assert P["63 zeros and 64 on lane 63"] == [0] * 63 + [64] and P["total 64: every lane its own owner"] == [1] * 64
    assert {sum(P[name]) for name in ("total 64: every lane its own owner", "total 65", "total 128", "total 4096")} == {64, 65, 128, 4096}
    assert [sum(w) > 0 for w in LW.waves(P["an idle wave between two"])] == [True, False, True]
    assert max(max(p) for p in P.values()) == 65 and len(P["three waves and a partial one"]) % 64 == 17


def test_lift_lengths_behind_a_short_prefix():
    solid = LW.lift_lengths([5] * 100)
    assert LW.stored_lengths(solid, *LW.LIFT_LENGTH_BOX, OUTSIDE, 8192, 354).tolist() == [5] * 70 + [0] * 30
    assert LW.stored_lengths(solid, *LW.LIFT_LENGTH_BOX, OUTSIDE, 60, 1 << 62).tolist() == [5] * 60 + [0] * 40
    assert LW.stored_lengths(solid, *LW.LIFT_LENGTH_BOX, OUTSIDE, 8192, 350).tolist() == [5] * 70 + [0] * 30, "room for exactly 70"
    assert LW.stored_lengths(solid, *LW.LIFT_LENGTH_BOX, OUTSIDE, 8192, 349).tolist() == [5] * 69 + [0] * 31, "one short of 70"


# ---- snapshot: the rectangles and the places of the changed columns ---------------------------------------------------------------------------------------------------

def test_snapshot_rectangles():
    for name, (rect, facts) in LW.SNAP_RECTS.items():
        n, groups, last, chunks = LW.snap_counts(rect)
        assert (n, groups, last) == facts, name
        assert rect[0] + rect[2] <= LW.SNAP_DIMS[0] and rect[1] + rect[3] <= LW.SNAP_DIMS[2]
        indices = LW.snap_scattered(rect)
        assert indices[-1] == n - 1 and len(set(indices)) == len(indices)
        for c in range(chunks):
            groups_of = {i // LW.SNAP_GROUP % 2 for i in indices if i // LW.SNAP_CHUNK == c}
            assert groups_of == {0, 1} or (c == chunks - 1 and n % LW.SNAP_CHUNK != 0 and groups_of), (name, c)
            assert c * LW.SNAP_CHUNK in indices and (min((c + 1) * LW.SNAP_CHUNK, n) - 1) in indices, "both ends of every chunk"
    assert sorted(facts[1] for _, facts in LW.SNAP_RECTS.values()) == [256, 257, 257, 512]
    assert LW.SNAP_DIMS[1] >> 5 == 1, "six levels"


def test_snapshot_places():
    rect = LW.SNAP_ONE_RECT
    places = {i: LW.snap_place(rect, i)[1:] for i in LW.SNAP_ONE_INDICES}
    assert places == {0: (0, 0, 0), 63: (0, 0, 63), 64: (0, 1, 0), 191: (0, 2, 63), 192: (0, 3, 0), 255: (0, 3, 63), 256: (1, 0, 0), 65535: (255, 3, 63),
                      65536: (256, 0, 0), 65789: (256, 3, 61)}
    assert LW.snap_counts(rect)[:3] == (65790, 257, 254)
    (ia, ya), (ib, yb) = LW.snap_box_pair(rect)
    (xa, za), ga, _, _ = LW.snap_place(rect, ia)
    (xb, zb), gb, _, _ = LW.snap_place(rect, ib)
    assert (ga, gb) == (0, 256) and xa < xb and za > zb and ya > yb
    terrain = LW.snap_terrain()
    heights = terrain.sum(axis=1)
    assert terrain.shape == LW.SNAP_DIMS and heights.min() == 5 and heights.max() == 19, "every voxel the cases paint or carve (y 1 .. 4) is solid"
    assert (terrain == (np.arange(32)[None, :, None] < heights[:, None, :])).all()
