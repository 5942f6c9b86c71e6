"""GPU: cvx_world_spread, cvx_world_nav_build and the component engine's cavity rule at the limits compiled into their kernels.

The continuation of tests/test_gpu_world_kernel_limits.py for the calls that came after it.  The constants are those of the .hip files:
  spread   the tile of 8 x 64 x 8 voxels and the kSpreadSweeps = 64 sweeps a tile makes per launch, after which it has to queue ITSELF again
           (spread_relax_kernel); the 32-bit word through which spread_seeds_kernel keeps a 16-bit minimum; the 64 words of an init workgroup and
           the 2048 elements of a finish workgroup
  nav      the kTileNodes = 1536 nodes (halo included) up to which nav_relax_kernel relaxes a tile of 16 x 16 cell columns in LDS and above which
           in global memory, the clamped halo rows at the grid's edge, the kSweeps = 64 sweeps per launch, and the rule's largest body
           (kNavMaxWidth = 8, kNavMaxHeight = 64: the w x w union walk of NavNextInterval)
  engine   the kernels of cvx_components.h instantiated for CavityRule at the wave shapes the pieces have there (one root per wave, a partial last
           wave, a root per node, lane 0 alone, 255 / 256 / 257 listed), a NON-ZERO bit carried through the wave reduction of stats_kernel for
           both rules, and thousands of unions that meet at one root (the comb)

Every case builds its volume in numpy (tests/limitworlds.py), asserts FROM THE VOLUME that the count it is named after is exactly that
(tests/test_limit_worlds_cpu.py asserts the same counts without a device), and only then compares the device's bytes and totals with the dense
models (spreadmodel, navmodel, piecesmodel, cavitymodel); after REMOVE / FILL every level is compared with the host-built LOD chain of the model's
world.  One fresh context per case.  The launch counts of the corridor cases are printed (pytest -s shows them); only the one the thread mapping
proves is asserted."""
import pytest

import cavitymodel
import limitworlds as LW
import piecesmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _dense
from test_gpu_world_cavities import _report as _cavities
from test_gpu_world_kernel_limits import _assert_world, _pieces_case, _uploaded
from test_gpu_world_nav import _field
from test_gpu_world_pieces import _report as _pieces
from test_gpu_world_spread import _check as _spread
from test_limit_worlds_cpu import assert_goals_cross_the_edge
from test_world_pieces_cpu import GROUND, OUTSIDE
from test_world_spread_cpu import AIR

pytestmark = pytest.mark.gpu

BOX = LW.PIECES_BOX
REMOVE, FILL = gpu.PIECES_REMOVE, gpu.CAVITIES_FILL
ARGB = 0xFF123456


# ---- spread: the tile that queues itself --------------------------------------------------------------------------------------------------------------

def _corridor(layers, seed_last=False, cut=65534):
    """The sealed corridor on a fresh context against the model -> (the model's summary, the device's launches)."""
    solid, cells = LW.spread_sealed_corridor(layers)
    count = LW.spread_corridor_facts(solid, cells)
    assert count == 36 * layers - 1 and LW.spread_row_sweeps(layers) > LW.SPREAD_SWEEPS
    ctx, ws = _uploaded(solid, _dense(solid))
    try:
        seed = cells[-1] if seed_last else cells[0]
        _, summary, expected = _spread(ctx, solid, (0, 0, 0), LW.SPREAD_DIMS, [seed], AIR, 0x3F, cut, f"{layers} layers")
        # no neighbour tile holds a passable voxel, so none ever falls and marks this one: only the tile's own flag brings it back after the 64
        # sweeps of a launch, and a row along z passes one cell per sweep (LW.spread_row_sweeps)
        assert summary["launches"] >= 2
        print(f"sealed corridor, {layers} layers, seed {'last' if seed_last else 'first'}, cut {cut}: launches {summary['launches']}, tile visits {summary['tileVisits']}")
        return expected, summary["launches"]
    finally:
        ctx.close()
        ws.close()


@pytest.mark.parametrize("layers", [32, 3])
def test_spread_a_corridor_sealed_inside_one_tile(layers):
    """1151 cells (32 layers) and 107 (3 layers, the shortest that needs more than 64 sweeps) inside tile (1, 0, 1)."""
    expected, _ = _corridor(layers)
    assert expected["reached"] == expected["passable"] == 36 * layers - 1 and expected["largestDistance"] == 36 * layers - 2


def test_spread_the_sealed_corridor_from_its_last_cell():
    """The value enters every row from the other end."""
    expected, _ = _corridor(32, seed_last=True)
    assert expected["reached"] == 1151 and expected["largestDistance"] == 1150


def test_spread_the_sealed_corridor_cut_in_the_middle():
    expected, _ = _corridor(32, cut=575)
    assert expected["reached"] == 576 and expected["largestDistance"] == 575 and expected["passable"] == 1151


# ---- spread: seeds that share a word, element and word counts around the workgroups ------------------------------------------------------------------------

@pytest.fixture()
def open_world():
    solid = LW.spread_open_world()
    ctx, ws = _uploaded(solid, _dense(solid))
    yield ctx, solid
    ctx.close()
    ws.close()


@pytest.mark.parametrize("parity", [0, 1])
def test_spread_seeds_on_two_voxels_of_one_word(open_world, parity):
    """64 seeds with distinct starts on each of the voxels y, y + 1 of one column, interleaved: in the even column the two 16-bit values share the
    word the compare-and-swap works on, in the odd one they lie in two.  No vertical step, so each voxel shows its own smallest start."""
    ctx, solid = open_world
    lo, hi, seeds, (a, b), index = LW.spread_shared_word(parity)
    assert (hi[1] - lo[1]) % 2 == 1 and index[1] == index[0] + 1 and index[0] % 2 == parity and len(seeds) == 128
    got, summary, expected = _spread(ctx, solid, lo, hi, seeds, AIR, 0x33, 200, f"parity {parity}")
    assert expected["seedsUsed"] == 128
    assert got[a[0] - lo[0], a[2] - lo[2], a[1] - lo[1]] == 3 and got[b[0] - lo[0], b[2] - lo[2], b[1] - lo[1]] == 40


@pytest.mark.parametrize("n", sorted(LW.SPREAD_ELEMENT_BOXES))
def test_spread_a_box_of_exactly_n_elements(open_world, n):
    """Around the 2048 elements of a finish workgroup (and the 256 of one of its trips)."""
    ctx, solid = open_world
    lo, hi = LW.SPREAD_ELEMENT_BOXES[n]
    assert LW.spread_counts(lo, hi)[0] == n and not solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].any()
    seeds = [(lo[0] + 1, hi[1] - 2, lo[2]), (hi[0] - 1, lo[1], hi[2] - 1, 5)]
    _, _, expected = _spread(ctx, solid, lo, hi, seeds, AIR, 0x3F, 1000, f"{n} elements")
    assert expected["reached"] == expected["passable"] == n and expected["seedsUsed"] == 2


@pytest.mark.parametrize("words", sorted(LW.SPREAD_WORD_BOXES))
def test_spread_a_box_of_exactly_n_words(open_world, words):
    """Around the 64 passable words of an init workgroup; the 65-word box sticks out of the world below."""
    ctx, solid = open_world
    lo, hi = LW.SPREAD_WORD_BOXES[words]
    assert LW.spread_counts(lo, hi)[1] == words
    seeds = [(lo[0], max(lo[1], 1), lo[2]), (hi[0] - 1, hi[1] - 1, hi[2] - 1, 3)]
    _, _, expected = _spread(ctx, solid, lo, hi, seeds, AIR, 0x3F, 1000, f"{words} words")
    assert expected["reached"] == expected["passable"] > 0 and expected["seedsUsed"] == 2


# ---- nav: 1536 nodes in LDS --------------------------------------------------------------------------------------------------------------------------------

def _nav_case(solid, call, goals, label, more_goals=()):
    """One build on a fresh context against the model: every voxel position's query and the summary -> (the model's steps and summary, launches).
    more_goals: further goal lists, each a build of its own on the same context, each against the model."""
    ctx, ws = _uploaded(solid, _dense(solid))
    try:
        field, want, summary = _field(ctx, solid, call, goals, label)
        launches = field.summary["launches"]
        field.close()
        for k, other in enumerate(more_goals):
            field, _, other_summary = _field(ctx, solid, call, other, f"{label}, goals {k + 2}")
            field.close()
            assert other_summary["reached"] == summary["reached"]
        return want, summary, launches
    finally:
        ctx.close()
        ws.close()


@pytest.mark.parametrize("total", [1535, 1536, 1537])
@pytest.mark.parametrize("name", sorted(LW.NAV_LIMIT_CASES))
def test_nav_a_tile_of_exactly(name, total):
    """The last two totals the tile path keeps in LDS and the first that relaxes in global memory, beside tiles of 324 nodes and fewer: in an
    interior tile, in the corner tile (halo rows and columns outside the grid) and in a box whose min corner is no multiple of 16.  One goal on
    the floor in the heavy tile's far corner, one a column beyond the halo of its +x edge, beside the slab columns: asserted from the model, more
    than 1000 slab nodes of the tile take their distance from the goal outside (the tile needs its halo's distances) and more than 500 nodes
    outside take theirs from the goal inside.  Built with both goals, and with the outside goal alone: then every way enters the tile."""
    tile, box_min = LW.NAV_LIMIT_CASES[name]
    solid, call, _ = LW.nav_limit_world(total, tile, box_min)
    totals = LW.nav_tile_totals(solid, call)
    assert totals[tile] == total and max(v for t, v in totals.items() if t != tile) <= 18 * 18
    assert totals[(0, 0)] == (total if tile == (0, 0) else 17 * 17)
    assert_goals_cross_the_edge(solid, call, tile)
    goals = LW.nav_limit_goals(call, tile)
    _, summary, _ = _nav_case(solid, call, goals, f"{name}, {total} nodes", more_goals=[goals[1:]])
    assert summary["goalsResolved"] == 2 and summary["reached"] == summary["nodes"] > 15000


def test_nav_heavy_columns_that_two_tiles_count():
    """Full slab columns on the heavy tile's last local x: the +x neighbour's halo holds them too.  The heavy tile has 1537 nodes (global memory),
    the neighbour exactly 1536 (LDS); the outside goal lies in the neighbour, so the ways into the heavy tile pass the shared columns."""
    solid, call, built = LW.nav_limit_world(1537, (2, 2), edge=14 * LW.NAV_SLABS, neighbour_total=1536)
    totals = LW.nav_tile_totals(solid, call)
    assert built == {(2, 2): 1537, (3, 2): 1536} and all(totals[t] == v for t, v in built.items())
    assert max(v for t, v in totals.items() if t not in built) <= 18 * 18
    assert_goals_cross_the_edge(solid, call, (2, 2))
    goals = LW.nav_limit_goals(call, (2, 2))
    _, summary, _ = _nav_case(solid, call, goals, "shared heavy columns", more_goals=[goals[1:]])
    assert summary["goalsResolved"] == 2 and summary["reached"] == summary["nodes"]


@pytest.mark.parametrize("slab_columns", [0, 36])
def test_nav_a_corridor_inside_one_tile(slab_columns):
    """135 cells in one tile, the goal at one end.  With 36 wall columns stacked with slabs the tile holds 1539 nodes and relaxes in global memory.
    Thread t of nav_relax_kernel owns local column (t / 16, t % 16): the 16 z of a row are lanes of ONE wave.  The corridor cell is the second
    node of each of their columns, so the wave relaxes the 16 cells in the same trip of RelaxColumn's loop, where every lane reads its neighbours'
    distances before any lane stores its own: a value passes one cell per sweep along a row, 8 rows x 15 hops = 120 sweeps, more than the
    kSweeps = 64 of a launch.  So launches >= 2 on both paths; the observed count is printed."""
    solid, call, cells = LW.nav_tile_corridor(slab_columns)
    totals = LW.nav_tile_totals(solid, call)
    assert len(cells) == 135 and totals[LW.NAV_CORRIDOR_TILE] == 324 + 135 + 30 * slab_columns
    assert (totals[LW.NAV_CORRIDOR_TILE] > LW.NAV_TILE_NODES) == (slab_columns > 0) and max(v for t, v in totals.items() if t != LW.NAV_CORRIDOR_TILE) <= LW.NAV_TILE_NODES
    assert LW.nav_corridor_row_sweeps(solid, call, cells) == 120 > LW.NAV_SWEEPS
    want, summary, launches = _nav_case(solid, call, [cells[0]], f"tile corridor, {slab_columns} slab columns")
    assert summary["reached"] == 135 and summary["largestDistance"] == 134 == want[cells[-1]]["distance"]
    print(f"nav tile corridor, tile total {totals[LW.NAV_CORRIDOR_TILE]}: launches {launches}")
    assert launches >= 2


@pytest.mark.parametrize("width,height,step_up,max_drop", LW.NAV_WIDE_RULES)
def test_nav_the_widest_and_the_tallest_body(width, height, step_up, max_drop):
    """Openings exactly 8 and 7 wide that leave exactly 64 and 63 clear: the body of 8 x 64 x 8 passes one, one voxel less of either opens another."""
    solid = LW.nav_wide_world()
    call = ((0, 0, 0), LW.NAV_WIDE_DIMS, width, height, step_up, max_drop, 0)
    want, summary, _ = _nav_case(solid, call, [LW.NAV_WIDE_GOAL], f"w {width} h {height}")
    LW.assert_wide_openings(want, width, height)
    assert summary["goalsResolved"] == 1 and summary["reached"] > 400


# ---- the component engine: the cavity rule at the wave shapes --------------------------------------------------------------------------------------------------

def _cavities_case(solid, enclosed, label, capacities=(0, 256, 8192), some=None, open_faces=0):
    """REPORT with every capacity, REPORT with a voxel limit that selects some, then FILL: summary and list against the model, every level after."""
    colour = _dense(solid)
    ctx, ws = _uploaded(solid, colour)
    try:
        for capacity in capacities:
            cavities, summary = _cavities(ctx, solid, *BOX, open_faces, 0, capacity, f"{label}, capacity {capacity}")
            assert summary["enclosedCavities"] == summary["selectedCavities"] == enclosed and len(cavities) == min(capacity, enclosed)
        if some is not None:
            _, summary = _cavities(ctx, solid, *BOX, open_faces, some, enclosed + 10, f"{label}, up to {some} voxels")
            assert 0 < summary["selectedCavities"] < enclosed == summary["enclosedCavities"]
        want, want_summary, _ = cavitymodel.analyse(solid, *BOX, open_faces, 0)
        got, summary, _ = ctx.world_cavities(*BOX, FILL, open_faces, 0, ARGB, 5, capacity=256)
        assert summary == want_summary and got.tobytes() == want[:256].tobytes(), f"{label}: FILL"
        _assert_world(ctx, *cavitymodel.fill(solid, colour, *BOX, open_faces, 0, ARGB), f"{label}: after FILL")
    finally:
        ctx.close()
        ws.close()


@pytest.mark.parametrize("name", sorted(LW.WAVE_SHAPES))
def test_cavities_at_the_wave_shape(name):
    """The complement of the pieces world of that shape, in a box inside rock: no region is open with openFaces 0, and no sky node interleaves."""
    build, count, some = LW.WAVE_SHAPES[name]
    solid = LW.complement(build())
    LW.assert_wave_shape(name, LW.node_cavities(solid, *BOX))
    assert LW.cavity_count(solid, *BOX) == count and solid[:, 63, :].all()
    _cavities_case(solid, count, name, capacities=(0, 256, count + 10), some=some)


# ---- a non-zero bit through the wave reduction, both rules ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lane", LW.BITS_LANES)
@pytest.mark.parametrize("anchor", [OUTSIDE, GROUND])
def test_pieces_one_node_anchors_a_wave_of_one_root(anchor, lane):
    """Every wave of the stats kernel has one root; ONE node of wave 4, at a middle lane or the last, holds the anchor bit (it alone touches the
    floor outside the box, or y = 0).  Its piece is anchored, the eight others float."""
    solid, box, column = LW.bars_one_node_down(lane, to_ground=anchor == GROUND)
    LW.assert_one_node_in_its_wave(LW.run_tops(solid, *box), LW.node_pieces(solid, *box), column, lane)
    colour = _dense(solid)
    ctx, ws = _uploaded(solid, colour)
    try:
        pieces, summary = _pieces(ctx, solid, *box, anchor, capacity=20, label=f"anchor {anchor}, lane {lane}")
        assert summary["anchoredPieces"] == 1 and summary["floatingPieces"] == 8 == len(pieces) and 2 * LW.BITS_ROW not in pieces["min"][:, 0].tolist()
        _, summary = _pieces(ctx, solid, *box, 0, capacity=20, label="no anchor")
        assert summary["floatingPieces"] == 9
        want, want_summary, _ = piecesmodel.analyse(solid, *box, anchor)
        pieces, summary, _ = ctx.world_pieces(*box, anchor, REMOVE, capacity=256)
        assert summary == want_summary and pieces.tobytes() == want.tobytes()
        _assert_world(ctx, *piecesmodel.remove(solid, colour, *box, anchor), f"anchor {anchor}, lane {lane}: after REMOVE")
    finally:
        ctx.close()
        ws.close()


@pytest.mark.parametrize("lane", LW.BITS_LANES)
def test_cavities_one_node_opens_a_wave_of_one_root(lane):
    """The same on the air side: ONE node of wave 4 reaches the +Y face of the box, with the outside of the world across it.  With +Y in openFaces
    its region is open and the eight others are enclosed; with the bit cleared all nine are enclosed."""
    solid, column = LW.bars_one_node_open(lane)
    LW.assert_one_node_in_its_wave(LW.air_tops(solid, *BOX), LW.node_cavities(solid, *BOX), column, lane)
    colour = _dense(solid)
    ctx, ws = _uploaded(solid, colour)
    try:
        cavities, summary = _cavities(ctx, solid, *BOX, 0x08, 0, 20, f"+Y open, lane {lane}")
        assert summary["openRegions"] == 1 and summary["enclosedCavities"] == 8 == len(cavities) and 2 * LW.BITS_ROW not in cavities["min"][:, 0].tolist()
        assert summary["openVoxels"] == 63 + 64 - (10 + LW.BITS_ROW % 3)
        _, summary = _cavities(ctx, solid, *BOX, 0, 0, 20, f"nothing open, lane {lane}")
        assert summary["openRegions"] == 0 and summary["enclosedCavities"] == 9
        want, want_summary, _ = cavitymodel.analyse(solid, *BOX, 0x08, 0)
        got, summary, _ = ctx.world_cavities(*BOX, FILL, 0x08, 0, ARGB, 5, capacity=256)
        assert summary == want_summary and got.tobytes() == want.tobytes()
        _assert_world(ctx, *cavitymodel.fill(solid, colour, *BOX, 0x08, 0, ARGB), f"lane {lane}: after FILL")
    finally:
        ctx.close()
        ws.close()


# ---- the comb: every union meets at one root ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("plate", [True, False])
def test_pieces_of_the_comb(plate):
    """992 bars of 64 nodes each, joined -- if at all -- by a plate at the last x: the unions of bar with bar all happen at the highest node
    indices, and every one of the 63 488 nodes along the bars has to end at the root at (0, 62, 0)."""
    solid, bars = LW.comb(plate)
    tops = LW.run_tops(solid, *BOX)
    assert tops[0].tolist() == [0, 62, 0] and int((tops[:, 0] < 63).sum()) == 63 * bars == int(solid[:63, 1:, :].sum())
    want, _, _ = piecesmodel.analyse(solid, *BOX, 0)
    assert (want["seed"][:, 0] == 0).all() and len(want) == (1 if plate else bars)
    _pieces_case(solid, 1 if plate else bars, f"comb, plate {plate}", capacities=(0, 256, bars + 10))


@pytest.mark.parametrize("plate", [True, False])
def test_cavities_of_the_comb(plate):
    solid, bars = LW.comb(plate)
    solid = LW.complement(solid)
    assert LW.air_tops(solid, *BOX)[0].tolist() == [0, 62, 0] and LW.cavity_count(solid, *BOX) == (1 if plate else bars)
    _cavities_case(solid, 1 if plate else bars, f"comb, plate {plate}", capacities=(0, 256, bars + 10))
