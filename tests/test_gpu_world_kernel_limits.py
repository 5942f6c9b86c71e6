"""GPU: cvx_world_light, cvx_world_settle and cvx_world_pieces at the size limits compiled into their kernels.

The limits are constants of the .hip files, not of the rules, so the host builds of the rules (tests/*_rules.cpp) cannot reach them: the 2048
entries of light_brick_kernel's LDS list (a tile slab of 16 x 16 x 32 voxels holds up to 8192 and is shaded in rounds), the 4096 nodes up to
which ONE workgroup relaxes a settle and the 8 sweeps per launch above it, the waves of cvxcomp::stats_kernel / settle_gap_kernel (one reduction
where a wave's nodes share a root, atomics per node otherwise) and the 256 pieces that come to the host with the totals.  The stats kernel,
the list and its head belong to the component engine (cvx_components.h), whose kernels are templates: cvx_world_cavities runs instantiations of
its own (CavityRule), which tests/test_gpu_world_kernel_limits_later.py takes through the same wave shapes -- with the cases that carry a non-zero
bit through the stats kernel's wave reduction, for both rules, and the limits of cvx_world_spread and cvx_world_nav_build.

Every case builds its volume in numpy (tests/limitworlds.py, no device needed) and asserts FROM THE VOLUME, before the device is called, that the
count it is named after is exactly that; only then are the device's results compared, byte for byte, with the dense models (lightmodel,
settlemodel, piecesmodel) and every level with the host-built LOD chain of the model's world.

cvx_world_stamp_mesh has a file of its own in the same manner: tests/test_gpu_world_stamp_limits.py (the pairs, the cap, the sort's tiles, the merge's
runs, the early exits)."""
import os

import pytest

import lightmodel
import limitworlds as LW
import piecesmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _dense
from test_gpu_world_copy import _assert_levels
from test_gpu_world_light import VARIANT, _levels, _light
from test_gpu_world_pieces import _report
from test_gpu_world_settle import _settle
from test_world_light_cpu import ALPHA, RGB, model_world
from test_world_pieces_cpu import GROUND, LARGEST

pytestmark = pytest.mark.gpu

REMOVE = gpu.PIECES_REMOVE


def _uploaded(solid, colour):
    ws = model_world(solid.shape, solid, colour)
    ctx = None
    try:
        ctx = gpu.Context(0)
        ctx.upload_world(ws)
    except BaseException:
        if ctx is not None:
            ctx.close()
        ws.close()
        raise
    return ctx, ws


def _assert_world(ctx, solid, colour, label):
    want = model_world(solid.shape, solid, colour)
    try:
        _assert_levels(ctx, want, want, 5, label)
    finally:
        want.close()


# ---- light: the rounds of the LDS list -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxels", [2047, 2048, 2049, 4097, 8192])
def test_light_with_a_tile_slab_of_exactly(voxels):
    """One tile slab holds exactly `voxels` solid voxels: one round with an entry to spare, a full list, one voxel into the second round, one into
    the third, and the full slab (four rounds).  The +x neighbour tile has no column, the last tile of every row is cut by the box's edge, and
    the roof puts voxels above the slab into the tile's columns (their colours come first in the blob).  TO_ALPHA, then TO_RGB on top of it."""
    solid, key = LW.light_world(voxels)
    counts = LW.light_slab_counts(solid, *LW.LIGHT_BOX)
    assert counts[key] == voxels, f"the slab holds {counts[key]} voxels"
    assert max(counts.values()) == voxels and sorted(counts.values())[-2] <= 2048 - 2, "the other slabs stay inside one round"
    hx, hz = LW.LIGHT_HOLE
    assert not any((hx, hz, y) in counts for y in range(64)) and not solid[hx:hx + 16, :, hz:hz + 16].any(), "the neighbour tile has no column"
    assert (51, 53, 0) in counts and counts[(51, 53, 0)] == 9 * 9, "the corner tile is cut by the box on both sides"
    colour = _dense(solid)
    calls = [lightmodel.params(*LW.LIGHT_BOX, sun_dir=(2, 3, 1), sun_level=150, sun_range=64, sky_level=90, sky_range=4, floor_level=20, target=target)
             for target in (ALPHA, RGB)]
    ctx, ws = _uploaded(solid, colour)
    try:
        try:
            for p in calls:
                assert _light(ctx, p) > 0.0
                colour = lightmodel.light(solid, colour, p)
                _assert_world(ctx, solid, colour, f"{voxels} voxels, target {p['target']}")
            product = _levels(ctx)
        finally:
            ctx.close()
        if os.path.exists(VARIANT):  # the -DCVX_LIGHT_RECORDS build: no brick, no list
            gpu.use_library(VARIANT)
            try:
                other = gpu.Context(0)
                try:
                    other.upload_world(ws)
                    for p in calls:
                        assert _light(other, p) > 0.0
                    assert _levels(other) == product, "the record-walking variant differs from the product"
                finally:
                    other.close()
            finally:
                gpu.use_library(None)
    finally:
        ws.close()


# ---- settle: one workgroup or launches of eight sweeps ---------------------------------------------------------------------------------------------

def _settle_case(solid, box, max_drop, label):
    """One settle on a fresh context against the model: the summary, pieces and drops (_settle), then every level -> the drops."""
    colour = _dense(solid)
    ctx, ws = _uploaded(solid, colour)
    try:
        after, summary, drops = _settle(ctx, solid, colour, *box, GROUND, max_drop=max_drop, label=label)
        assert summary["fallenPieces"] > 0
        _assert_world(ctx, *after, label)
        return drops.tolist()
    finally:
        ctx.close()
        ws.close()


@pytest.mark.parametrize("nodes", [4095, 4096, 4097])
def test_settle_a_box_of_exactly(nodes):
    """The box holds exactly `nodes` nodes (solid runs clipped to it): the last two sizes one workgroup relaxes, and the first one that goes
    through the launches of eight sweeps."""
    solid = LW.settle_nodes(nodes)
    assert LW.node_count(solid, *LW.SETTLE_NODE_BOX) == nodes
    drops = _settle_case(solid, LW.SETTLE_NODE_BOX, 0, f"{nodes} nodes")
    assert drops.count(1) == 1 and max(drops) == 6, "the stack of three (drops 1, 3, 6) is among the pieces"


@pytest.mark.parametrize("pieces,max_drop", [(7, 0), (8, 0), (9, 0), (16, 0), (17, 0), (9, 5)])
def test_settle_a_stack_of_exactly(pieces, max_drop):
    """`pieces` slabs that rest on one another after the fall, a chain of `pieces` constraints: the stack heights on both sides of one and two
    times the 8 sweeps of a relax launch.  Which sweep finds "nothing changed" is not observable from outside (within a sweep the waves run
    in no fixed order, so a drop can travel several slabs at once) and is not asserted; what is asserted is that the drops are the model's and
    the same through both relax paths: once in a box of fewer than 4096 nodes, which one workgroup relaxes, and once with the whole world as
    the box (the floor's 16 384 columns lift it above 4096 nodes), which goes through the launches.  (9, 5): maxDrop smaller than the deepest
    chain."""
    solid, chain = LW.settle_stack(pieces)
    small, whole = LW.node_count(solid, *LW.SETTLE_SMALL_BOX), LW.node_count(solid, *LW.SETTLE_WHOLE)
    assert small < 4096 < whole, (small, whole)
    for box in (LW.SETTLE_SMALL_BOX, LW.SETTLE_WHOLE):
        assert LW.piece_count(solid, *box) == pieces + 1, "the floor and the slabs"
    assert len(chain) == pieces and max(chain) == sum(LW.stack_gaps(pieces)) and (max_drop == 0 or max_drop < max(chain))
    want = [min(d, max_drop) for d in chain] if max_drop else chain
    one = _settle_case(solid, LW.SETTLE_SMALL_BOX, max_drop, f"{pieces} slabs, one workgroup")
    many = _settle_case(solid, LW.SETTLE_WHOLE, max_drop, f"{pieces} slabs, launches")
    assert one == many == want


# ---- pieces: the waves of the stats kernel, the head of the list ----------------------------------------------------------------------------------------

def _pieces_case(solid, floating, label, capacities=(0, 256, 8192)):
    """REPORT with every capacity and no anchor, REPORT with LARGEST, then REMOVE: the summary and the list against the model, every level after."""
    box = LW.PIECES_BOX
    assert LW.piece_count(solid, *box) == floating
    colour = _dense(solid)
    ctx, ws = _uploaded(solid, colour)
    try:
        for capacity in capacities:
            pieces, summary = _report(ctx, solid, *box, 0, capacity=capacity, label=f"{label}, capacity {capacity}")
            assert summary["floatingPieces"] == floating and len(pieces) == min(capacity, floating)
        _, summary = _report(ctx, solid, *box, LARGEST, capacity=floating + 10, label=f"{label}, largest")
        assert summary["floatingPieces"] == floating - 1 and summary["anchoredPieces"] == 1
        want, want_summary, _ = piecesmodel.analyse(solid, *box, 0)
        pieces, summary, _ = ctx.world_pieces(*box, 0, REMOVE, capacity=256)
        assert summary == want_summary and pieces.tobytes() == want[:256].tobytes(), f"{label}: REMOVE"
        _assert_world(ctx, *piecesmodel.remove(solid, colour, *box, 0), f"{label}: after REMOVE")
    finally:
        ctx.close()
        ws.close()


def test_pieces_where_every_wave_is_one_piece():
    solid = LW.pieces_bars()
    roots = LW.node_pieces(solid, *LW.PIECES_BOX)
    assert len(roots) == 9 * 64 and all(len(set(w)) == 1 for w in LW.waves(roots)) and len(set(roots)) == 9
    _pieces_case(solid, 9, "one piece per wave")


@pytest.mark.parametrize("last", [1, 63])
def test_pieces_with_a_partial_last_wave(last):
    """64 k + 1 nodes (the last wave has one live lane) and 64 k + 63."""
    solid = LW.pieces_bars(last=last)
    roots = LW.node_pieces(solid, *LW.PIECES_BOX)
    assert len(roots) == 8 * 64 + last and len(LW.waves(roots)[-1]) == last and all(len(set(w)) == 1 for w in LW.waves(roots))
    _pieces_case(solid, 9, f"{len(roots)} nodes")


def test_pieces_where_every_node_is_its_own_piece():
    solid = LW.pieces_checkerboard()
    roots = LW.node_pieces(solid, *LW.PIECES_BOX)
    assert len(roots) == 2048 and len(set(roots)) == 2048
    _pieces_case(solid, 2048, "a piece per node")


def test_pieces_where_lane_0_differs_from_the_rest_of_its_wave():
    solid = LW.pieces_lone_leader()
    roots = LW.node_pieces(solid, *LW.PIECES_BOX)
    assert len(roots) == 6 * 64
    for w in LW.waves(roots):
        assert len(w) == 64 and w[0] != w[1] and len(set(w[1:])) == 1
    _pieces_case(solid, 12, "lane 0 alone")


@pytest.mark.parametrize("floating", [255, 256, 257, 513])
def test_pieces_with_exactly(floating):
    """`floating` floating pieces around the 256 that travel with the totals; capacities of 0, 256 and more than the count."""
    solid = LW.pieces_checkerboard(floating)
    assert LW.node_count(solid, *LW.PIECES_BOX) == floating
    _pieces_case(solid, floating, f"{floating} pieces", capacities=(0, 256, floating + 10))
