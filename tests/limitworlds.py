"""Test infrastructure (numpy only, no device): the volumes of tests/test_gpu_world_kernel_limits.py and the counts they are named after.

The size limits of the world kernels are constants of the .hip files (the LDS list of light_brick_kernel, the node count up to which one
workgroup relaxes a settle, the sweeps per relax launch, the waves of cvxcomp::stats_kernel, the list head that travels with the totals).  Every
builder here returns a volume TOGETHER with the count that decides which side of such a limit it lies on, computed from the volume alone by the
counting functions below; the GPU test asserts the count before it calls the device."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

SIX = ndimage.generate_binary_structure(3, 1)
TILE, SLAB, WAVE = 16, 32, 64


def clip(dims, box_min, box_max):
    lo = [max(int(box_min[a]), 0) for a in range(3)]
    hi = [min(int(box_max[a]), dims[a]) for a in range(3)]
    assert all(lo[a] < hi[a] for a in range(3))
    return lo, hi


# ---- counting ------------------------------------------------------------------------------------------------------------------------------------

def light_slab_counts(solid, box_min, box_max):
    """{(tile x, tile z, slab y): solid voxels inside the box} for every tile slab the light kernel walks: tiles of 16 x 16 columns from the
    clipped box's (x0, z0); per tile, slabs of 32 voxels from max(box y0, the lowest voxel of the tile's columns) up to min(box y1, their highest
    voxel + 1).  A tile without a column has no slab."""
    lo, hi = clip(solid.shape, box_min, box_max)
    out = {}
    for tx in range(lo[0], hi[0], TILE):
        for tz in range(lo[2], hi[2], TILE):
            columns = solid[tx:min(tx + TILE, hi[0]), :, tz:min(tz + TILE, hi[2])]
            ys = np.nonzero(columns.any(axis=(0, 2)))[0]
            if len(ys) == 0:
                continue
            y_lo, y_hi = max(lo[1], int(ys[0])), min(hi[1], int(ys[-1]) + 1)
            for y in range(y_lo, y_hi, SLAB):
                out[(tx, tz, y)] = int(columns[:, y:min(y + SLAB, y_hi), :].sum())
    return out


def run_tops(solid, box_min, box_max):
    """The nodes of a box in the device's order: the top voxel (x, y, z) of every maximal vertical solid run of the volume clipped to the box,
    columns in x then z order, top-down inside a column."""
    lo, hi = clip(solid.shape, box_min, box_max)
    sub = solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    top = sub.copy()
    top[:, :-1, :] &= ~sub[:, 1:, :]
    x, y, z = np.nonzero(top)
    order = np.lexsort((-y, z, x))
    return np.stack([x[order] + lo[0], y[order] + lo[1], z[order] + lo[2]], axis=1)


def node_count(solid, box_min, box_max):
    return len(run_tops(solid, box_min, box_max))


def node_pieces(solid, box_min, box_max):
    """The piece (a label of scipy.ndimage.label over the box, face contact) of every node, in the device's node order."""
    lo, hi = clip(solid.shape, box_min, box_max)
    labels, _ = ndimage.label(solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], structure=SIX)
    tops = run_tops(solid, box_min, box_max)
    return labels[tops[:, 0] - lo[0], tops[:, 1] - lo[1], tops[:, 2] - lo[2]]


def piece_count(solid, box_min, box_max):
    lo, hi = clip(solid.shape, box_min, box_max)
    return int(ndimage.label(solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], structure=SIX)[1])


def waves(values):
    """values cut into the waves of a launch with one thread per node: 64 at a time, the last one partial."""
    return [values[at:at + WAVE] for at in range(0, len(values), WAVE)]


# ---- light: the voxels of one tile slab ----------------------------------------------------------------------------------------------------------

LIGHT_DIMS = (64, 64, 64)
LIGHT_BOX = ((3, 0, 5), (60, 64, 62))   # tiles from (3, 5): three whole ones and one 9 (x) / 9 (z) columns wide per row, cut by the box's edge
LIGHT_TILE = (19, 21)                   # the tile that is filled
LIGHT_HOLE = (35, 21)                   # its +x neighbour: no column at all


def light_world(voxels):
    """A floor at y = 0; the slab y 0 .. 31 of the tile at LIGHT_TILE holds exactly `voxels` solid voxels (256 .. 8192: the floor's 256, then whole
    layers from y = 31 downwards and one partial layer, so that columns below the partial layer have two runs); a roof at y = 40 over the tile
    puts voxels above the slab into its columns; the tile at LIGHT_HOLE has no column.  -> (solid, the key of the slab in light_slab_counts)."""
    assert TILE * TILE <= voxels <= TILE * TILE * SLAB
    solid = np.zeros(LIGHT_DIMS, dtype=bool)
    solid[:, 0, :] = True
    tx, tz = LIGHT_TILE
    rest, y = voxels - TILE * TILE, SLAB - 1
    while rest > 0:
        layer = min(rest, TILE * TILE)
        cells = np.zeros(TILE * TILE, dtype=bool)
        cells[:layer] = True
        solid[tx:tx + TILE, y, tz:tz + TILE] = cells.reshape(TILE, TILE)
        rest -= layer
        y -= 1
    solid[tx:tx + TILE, 40, tz:tz + TILE] = True
    solid[tx + 3, 41:50, tz + 5] = True  # (and a pole: the roof's slab is not one layer)
    hx, hz = LIGHT_HOLE
    solid[hx:hx + TILE, :, hz:hz + TILE] = False
    return solid, (tx, tz, 0)


# ---- settle: nodes in the box, pieces in a stack ----------------------------------------------------------------------------------------------------

SETTLE_DIMS = (128, 64, 128)
SETTLE_SMALL_BOX = ((32, 0, 32), (56, 64, 56))
SETTLE_WHOLE = ((0, 0, 0), SETTLE_DIMS)
SETTLE_NODE_BOX = ((0, 0, 0), (64, 64, 63))  # 4032 floor columns


def stack_gaps(pieces):
    return [1 + k % 3 for k in range(pieces)]


def settle_stack(pieces):
    """A floor and a stack of `pieces` slabs of 2 x 2 x 1 voxels around column (40, 40), slab k lying stack_gaps(pieces)[k] voxels of air above
    slab k - 1 (slab 0 above the floor) and shifted by one column in x against it, so that half of it hangs over the slab two below (or the
    floor): a looser constraint, which the relaxation has to lower along the chain.  Slab k falls gaps[0] + .. + gaps[k].
    -> (solid, the drops in list order: the highest slab first)."""
    solid = np.zeros(SETTLE_DIMS, dtype=bool)
    solid[:, 0, :] = True
    y, drops, total = 0, [], 0
    for k, gap in enumerate(stack_gaps(pieces)):
        y += gap + 1
        total += gap
        x = 40 + k % 2
        solid[x:x + 2, y, 40:42] = True
        drops.append(total)
    assert y < SETTLE_DIMS[1]
    # the list is in seed order: first column in (x, z) order, there the highest voxel.  Even slabs start at x = 40, odd ones at x = 41.
    order = sorted(range(pieces), key=lambda k: (k % 2, -k))
    return solid, [drops[k] for k in order]


def settle_nodes(nodes):
    """A floor, a stack of three slabs and single floating voxels at every second column, as many as bring SETTLE_NODE_BOX to exactly `nodes`
    nodes.  -> solid"""
    solid, _ = settle_stack(3)
    pads = nodes - node_count(solid, *SETTLE_NODE_BOX)
    assert 0 < pads < 400
    for k in range(pads):
        solid[2 + 2 * (k % 16), 3 + k % 5, 2 + 2 * (k // 16)] = True
    return solid


# ---- pieces: what the waves of the stats kernel hold, and the list head ---------------------------------------------------------------------------------

PIECES_DIMS = (64, 64, 64)
PIECES_BOX = ((0, 1, 0), PIECES_DIMS)  # above the floor (y = 0), which lies outside the box: with no anchor bit everything in the box floats


def _floor(dims):
    solid = np.zeros(dims, dtype=bool)
    solid[:, 0, :] = True
    return solid


def pieces_bars(last=WAVE, rows=9):
    """Bars along z (64 columns = 64 nodes = one wave) on every second row x, the last one `last` columns long: every wave belongs to one piece,
    and the node count is 64 * (rows - 1) + last."""
    solid = _floor(PIECES_DIMS)
    for r in range(rows):
        solid[2 * r, 10 + r % 3, 0:(WAVE if r + 1 < rows else last)] = True
    return solid


def pieces_checkerboard(count=None):
    """Single voxels on the cells of a checkerboard (no face contact), the first `count` of them in node order (None: all 2048): every node is
    its own piece."""
    solid = _floor(PIECES_DIMS)
    x, z = np.nonzero((np.arange(64)[:, None] + np.arange(64)[None, :]) % 2 == 0)
    if count is not None:
        assert count <= len(x)
        x, z = x[:count], z[:count]
    solid[x, 10 + (x + z) % 7, z] = True
    return solid


def pieces_lone_leader(rows=6):
    """On every second row x: a lone voxel in column z = 0 and a bar over z = 1 .. 63 at another height: lane 0 of every wave has a piece of its
    own, the 63 other lanes share one."""
    solid = _floor(PIECES_DIMS)
    for r in range(rows):
        solid[2 * r, 20, 0] = True
        solid[2 * r, 10, 1:WAVE] = True
    return solid
