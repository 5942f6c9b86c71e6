"""Test infrastructure (numpy and scipy only, no device): the volumes of tests/test_gpu_world_kernel_limits.py,
tests/test_gpu_world_kernel_limits_later.py and tests/test_gpu_world_kernel_limits_newest.py and the counts they are named after
(tests/test_limit_worlds_cpu.py checks the later and the newest ones on the CPU).

The size limits of the world kernels are constants of the .hip files (the LDS list of light_brick_kernel, the node count up to which one
workgroup relaxes a settle, the sweeps per relax launch, the waves of cvxcomp::stats_kernel, the list head that travels with the totals; the
spread tile and its sweeps per launch, the nodes a nav tile keeps in LDS, the widest and tallest nav body; the waves of lift_moments_kernel and
lift_write_kernel, the 256 columns of a snapshot diff's count workgroup, the 256 partials a thread of its reduce kernel steps over).  Every
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


def pieces_bars(last=WAVE, rows=9, deep=False):
    """Bars along z (64 columns = 64 nodes = one wave) on every second row x, the last one `last` columns long: every wave belongs to one piece,
    and the node count is 64 * (rows - 1) + last.  deep: the bars of the odd rows are two voxels high (the same nodes, twice the voxels: sizes
    that a voxel limit can tell apart)."""
    solid = _floor(PIECES_DIMS)
    for r in range(rows):
        y = 10 + r % 3
        solid[2 * r, y:y + (2 if deep and r % 2 else 1), 0:(WAVE if r + 1 < rows else last)] = True
    return solid


def pieces_checkerboard(count=None, deep=False):
    """Single voxels on the cells of a checkerboard (no face contact), the first `count` of them in node order (None: all 2048): every node is
    its own piece.  deep: the cells with (x + z) % 7 == 0 are two voxels high."""
    solid = _floor(PIECES_DIMS)
    x, z = np.nonzero((np.arange(64)[:, None] + np.arange(64)[None, :]) % 2 == 0)
    if count is not None:
        assert count <= len(x)
        x, z = x[:count], z[:count]
    solid[x, 10 + (x + z) % 7, z] = True
    if deep:
        tall = (x + z) % 7 == 0
        solid[x[tall], 11, z[tall]] = True
    return solid


def pieces_lone_leader(rows=6):
    """On every second row x: a lone voxel in column z = 0 and a bar over z = 1 .. 63 at another height: lane 0 of every wave has a piece of its
    own, the 63 other lanes share one."""
    solid = _floor(PIECES_DIMS)
    for r in range(rows):
        solid[2 * r, 20, 0] = True
        solid[2 * r, 10, 1:WAVE] = True
    return solid


# ---- the air side: the nodes of the cavity rule ------------------------------------------------------------------------------------------------------

def air_tops(solid, box_min, box_max):
    """run_tops on the air side: the top voxel of every maximal vertical AIR run of the volume clipped to the box (the nodes of the cavity rule),
    in the device's order."""
    return run_tops(~solid, box_min, box_max)


def node_cavities(solid, box_min, box_max):
    """node_pieces on the air side: the region (a label of scipy.ndimage.label over the box's air, face contact) of every air node, in the
    device's node order."""
    return node_pieces(~solid, box_min, box_max)


def cavity_count(solid, box_min, box_max):
    return piece_count(~solid, box_min, box_max)


def complement(solid):
    """Rock where `solid` has air and the other way round, y = 0 kept solid: inside PIECES_BOX the air nodes of the result are the solid nodes of
    `solid`, and the box lies inside rock (no sky node interleaves: the world's top is the box's top, and rock reaches it)."""
    out = ~solid
    out[:, 0, :] = True
    return out


def node_at(tops, x, z):
    """The index of the one node of column (x, z) in a list of run_tops / air_tops."""
    at = np.flatnonzero((tops[:, 0] == x) & (tops[:, 2] == z))
    assert len(at) == 1, f"column ({x}, {z}) has {len(at)} nodes"
    return int(at[0])


# ---- one node that carries a bit into a wave of one root ----------------------------------------------------------------------------------------------

BITS_ROW = 4           # the bar (= the wave) that holds the node
BITS_LANES = (29, 63)  # a middle lane and the last one


def bars_one_node_down(lane, to_ground=False):
    """pieces_bars with the node `lane` of bar BITS_ROW extended down to y = 1, where it touches the floor outside PIECES_BOX (the anchor OUTSIDE);
    to_ground: without the floor and down to y = 0 (the anchor GROUND, the box the whole world).  -> (solid, box, the node's (x, z))."""
    solid = pieces_bars()
    x, top = 2 * BITS_ROW, 10 + BITS_ROW % 3
    if to_ground:
        solid[:, 0, :] = False
        solid[x, 0:top, lane] = True
        return solid, ((0, 0, 0), PIECES_DIMS), (x, lane)
    solid[x, 1:top, lane] = True
    return solid, PIECES_BOX, (x, lane)


def bars_one_node_open(lane):
    """complement(pieces_bars()) with the air node `lane` of bar BITS_ROW extended up to the world's top, the +Y face of PIECES_BOX, with air (the
    outside of the world) across it.  -> (solid, the node's (x, z))."""
    solid = complement(pieces_bars())
    x, y = 2 * BITS_ROW, 10 + BITS_ROW % 3
    solid[x, y:, lane] = False
    return solid, (x, lane)


# ---- the comb: every union meets at one root ------------------------------------------------------------------------------------------------------------

def comb(plate=True):
    """In 64^3 above a floor: bars one voxel thick along x at every second y (2 .. 62) and z (0 .. 62).  Every voxel along a bar is a node of its
    own, and a bar's smallest node index is the one at x = 0.  plate: all bars are joined by a plate at the LAST x only, so every union of bar
    with bar meets at the end with the highest node indices.  -> (solid, bars)."""
    solid = _floor(PIECES_DIMS)
    ys, zs = np.arange(2, 63, 2), np.arange(0, 63, 2)
    solid[:, ys[:, None], zs[None, :]] = True
    if plate:
        solid[63, 2:63, :] = True
    return solid, len(ys) * len(zs)


# ---- spread: a corridor sealed inside one tile ----------------------------------------------------------------------------------------------------------

SPREAD_DIMS = (32, 64, 32)
SPREAD_TILE = (8, 64, 8)
SPREAD_SWEEPS = 64


def spread_sealed_corridor(layers):
    """A solid world with one corridor that lies wholly inside spread tile (1, 0, 1) = x and z 8 .. 15, all y.  On every even y (`layers` of them)
    four rows along z at x = 8, 10, 12, 14, joined at alternating ends by one cell at the odd x between them; layers are joined by one cell at the
    odd y between them.  -> (solid, the cells in the corridor's order, (x, y, z) each)."""
    assert 1 <= layers <= 32
    solid = np.ones(SPREAD_DIMS, dtype=bool)
    layer = []
    for k, x in enumerate((8, 10, 12, 14)):
        zs = range(8, 16) if k % 2 == 0 else range(15, 7, -1)
        layer.extend((x, z) for z in zs)
        if k < 3:
            layer.append((x + 1, layer[-1][1]))
    cells = []
    for n in range(layers):
        walk = layer if n % 2 == 0 else layer[::-1]
        cells.extend((x, 2 * n, z) for x, z in walk)
        if n + 1 < layers:
            cells.append((walk[-1][0], 2 * n + 1, walk[-1][1]))
    c = np.array(cells)
    solid[c[:, 0], c[:, 1], c[:, 2]] = False
    return solid, cells


def spread_row_sweeps(layers):
    """The sweeps the sealed corridor needs at the least.  The relax kernel's thread t owns 16 y of column t / 4 of the tile, column c = local
    (x, z) = (c / 8, c % 8): the 8 z of one x at one y are lanes of ONE wave, and a wave reads its neighbours beside it before any of its lanes
    writes.  So a value moves one cell per sweep along a row along z: 7 hops a row, 4 rows a layer."""
    return 7 * 4 * layers


def spread_corridor_facts(solid, cells):
    """What the sealed-corridor cases assert from the volume: the cells are distinct, they are all the air there is, all of it lies in tile
    (1, 0, 1), and consecutive cells are face neighbours."""
    c = np.array(cells)
    assert len(set(cells)) == len(cells) == int((~solid).sum())
    assert (c[:, 0] // SPREAD_TILE[0] == 1).all() and (c[:, 2] // SPREAD_TILE[2] == 1).all() and c[:, 1].max() < SPREAD_TILE[1]
    assert (np.abs(np.diff(c, axis=0)).sum(axis=1) == 1).all()
    return len(cells)


def spread_counts(lo, hi):
    """(elements, passable words) of a spread box: X * Y * Z voxels, and a word per column and chunk of 64 y."""
    sx, sy, sz = (hi[a] - lo[a] for a in range(3))
    return sx * sy * sz, sx * sz * -(-sy // 64)


SPREAD_TALL = (32, 256, 32)
# n around the 2048 elements of a finish workgroup (8 per thread), and words around the 64 of an init workgroup (16 per wave)
SPREAD_ELEMENT_BOXES = {2047: ((3, 5, 7), (26, 94, 8)), 2048: ((0, 9, 4), (32, 73, 5)), 4095: ((2, 3, 28), (17, 94, 31)), 4096: ((0, 100, 2), (32, 228, 3)),
                        4097: ((9, 10, 11), (26, 251, 12))}
SPREAD_WORD_BOXES = {63: ((5, 20, 31), (26, 150, 32)), 64: ((11, 1, 13), (19, 65, 21)), 65: ((14, -1, 3), (27, 256, 4))}


def spread_open_world():
    """The 32 x 256 x 32 world with nothing but a floor at y = 0."""
    return _floor(SPREAD_TALL)


def spread_shared_word(parity):
    """A box with an odd y size (Y = 9) over the open world and two voxels y, y + 1 (y even in the box) of one column: in a column of even index
    their 16-bit values share a 32-bit word, in one of odd index they straddle two.  64 seeds on each, distinct starts, interleaved; the smallest
    start of either voxel stands in the middle of the list.  -> (lo, hi, seeds, the two voxels, their element indices)."""
    lo, hi = (4, 3, 6), (9, 12, 11)
    sy, sz = hi[1] - lo[1], hi[2] - lo[2]
    bx, bz = 2, 2 + parity  # column index 2 * 5 + 2 + parity: 12 or 13, times Y = 9
    a, b = (lo[0] + bx, lo[1] + 4, lo[2] + bz), (lo[0] + bx, lo[1] + 5, lo[2] + bz)
    index = [((bx * sz + bz) * sy + v[1] - lo[1]) for v in (a, b)]
    rng = np.random.default_rng(7 + parity)
    starts_a, starts_b = 3 + rng.permutation(64), 40 + rng.permutation(64)
    for starts in (starts_a, starts_b):  # the smallest one neither first nor last
        k = int(np.argmin(starts))
        starts[[k, 31]] = starts[[31, k]]
    seeds = []
    for sa, sb in zip(starts_a, starts_b):
        seeds += [a + (int(sa),), b + (int(sb),)]
    return lo, hi, seeds, (a, b), index


# ---- nav: the nodes of a tile ----------------------------------------------------------------------------------------------------------------------------

NAV_DIMS = (128, 64, 128)
NAV_TILE, NAV_TILE_NODES, NAV_SWEEPS = 16, 1536, 64
NAV_SLAB_RULE = (1, 1, 1, 4096, 0)  # width, height, stepUp, maxDrop, maxSteps: a column with k slabs has k + 1 nodes
NAV_SLABS = 31                      # the slabs a column of 64 voxels holds: y = 2, 4, .. 62


def nav_column_nodes(solid, call):
    """The nodes of every cell column of a nav call, as nav_count_kernel counts them: an int array over the cell grid (the clipped box shrunk by
    width - 1 in x and z), and the grid's (x0, z0).  A node is a stand cell: floor below, `height` clear voxels (the union of the body's w x w
    columns), its floor inside the box's y range."""
    import navmodel

    box_min, box_max, width, height = call[0], call[1], call[2], call[3]
    lo, hi = clip(solid.shape, box_min, box_max)
    size_x, size_z = hi[0] - lo[0] - width + 1, hi[2] - lo[2] - width + 1
    assert size_x > 0 and size_z > 0
    cells = navmodel.stand_cells(solid, width, height)
    keep = (cells[:, 0] >= lo[0]) & (cells[:, 0] < lo[0] + size_x) & (cells[:, 2] >= lo[2]) & (cells[:, 2] < lo[2] + size_z) & (cells[:, 1] >= lo[1]) & (cells[:, 1] < hi[1])
    counts = np.zeros((size_x, size_z), dtype=np.int64)
    np.add.at(counts, (cells[keep, 0] - lo[0], cells[keep, 2] - lo[2]), 1)
    return counts, (lo[0], lo[2])


def nav_tile_totals(solid, call):
    """{(tile x, tile z): nodes} as nav_relax_kernel counts them: tiles of 16 x 16 cell columns numbered from the cell grid's own (x0, z0), each
    with its one-column halo clipped to the grid."""
    counts, _ = nav_column_nodes(solid, call)
    size_x, size_z = counts.shape
    out = {}
    for tx in range(-(-size_x // NAV_TILE)):
        for tz in range(-(-size_z // NAV_TILE)):
            cx, cz = tx * NAV_TILE, tz * NAV_TILE
            out[(tx, tz)] = int(counts[max(cx - 1, 0):min(cx + NAV_TILE + 1, size_x), max(cz - 1, 0):min(cz + NAV_TILE + 1, size_z)].sum())
    return out


def nav_tile_box(call, tile):
    """The box whose cell grid is the tile and its halo (width 1): what navmodel.analyse counts `nodes` over for that tile."""
    box_min, box_max = call[0], call[1]
    x0, z0 = max(box_min[0], 0) + tile[0] * NAV_TILE, max(box_min[2], 0) + tile[1] * NAV_TILE
    return (max(x0 - 1, box_min[0], 0), box_min[1], max(z0 - 1, box_min[2], 0)), (min(x0 + NAV_TILE + 1, box_max[0]), box_max[1], min(z0 + NAV_TILE + 1, box_max[2]))


def _stack_slabs(solid, columns, extra, base=0):
    """`extra` one-voxel slabs over `columns` ((x, z) each), column after column: full columns first, the rest in the last one.  Slab j of a column
    lies at y = base + 2 (j + 1): one more node of height 1 each."""
    room = (solid.shape[1] - 1 - base) // 2
    assert 0 <= extra <= room * len(columns), (extra, room, len(columns))
    for x, z in columns:
        k = min(extra, room)
        if k == 0:
            break
        solid[x, base + 2:base + 2 * k + 1:2, z] = True
        extra -= k


def nav_limit_world(total, tile, box_min=(0, 0, 0), edge=0, neighbour_total=None):
    """A floor at y = 0 and one-voxel slabs at y = 2, 4, .. over columns of tile `tile` (numbered from the box's min corner), so that the tile, with
    its halo, holds exactly `total` nodes under NAV_SLAB_RULE.  The slabs stand on interior columns (local 1 .. 14, in no neighbour's halo), but
    for `edge` of them, which stand on the tile's last local x (local z 1 .. 14): the +x neighbour's halo counts those too, and with
    neighbour_total that tile is brought to exactly that many nodes by slabs on its own interior columns.
    -> (solid, the call, {tile: the total it is built for})."""
    solid = _floor(NAV_DIMS)
    call = (tuple(box_min), NAV_DIMS) + NAV_SLAB_RULE
    size = [NAV_DIMS[a] - box_min[a] for a in (0, 2)]

    def base_of(t):  # the floor's nodes: the tile's columns and its halo, clipped to the grid
        spans = [min(t[a] * NAV_TILE + NAV_TILE + 1, size[a]) - max(t[a] * NAV_TILE - 1, 0) for a in (0, 1)]
        return spans[0] * spans[1]

    def interior(t):
        x0, z0 = box_min[0] + t[0] * NAV_TILE, box_min[2] + t[1] * NAV_TILE
        return [(x0 + lx, z0 + lz) for lx in range(NAV_TILE - 2, 0, -1) for lz in range(1, NAV_TILE - 1)]  # from the +x side: beside nav_limit_goals' outside goal

    x0, z0 = box_min[0] + tile[0] * NAV_TILE, box_min[2] + tile[1] * NAV_TILE
    _stack_slabs(solid, [(x0 + NAV_TILE - 1, z0 + lz) for lz in range(1, NAV_TILE - 1)], edge)
    _stack_slabs(solid, interior(tile), total - base_of(tile) - edge)
    built = {tuple(tile): total}
    if neighbour_total is not None:
        other = (tile[0] + 1, tile[1])
        _stack_slabs(solid, interior(other), neighbour_total - base_of(other) - edge)
        built[other] = neighbour_total
    return solid, call, built


NAV_LIMIT_CASES = {"interior tile": ((2, 2), (0, 0, 0)), "corner tile": ((0, 0), (0, 0, 0)), "box from (5, 0, 9)": ((2, 2), (5, 0, 9))}  # name -> (tile, box_min)


def nav_limit_goals(call, tile):
    """Two goals on the floor: one inside the heavy tile, in its -x, -z corner (local (1, 1)), and one outside, one column beyond the halo of its
    +x edge (local x = 17), three steps from the slab columns.  Ways to the first leave the tile, ways to the second enter it."""
    x0, z0 = call[0][0] + tile[0] * NAV_TILE, call[0][2] + tile[1] * NAV_TILE
    return [(x0 + 1, 1, z0 + 1), (x0 + NAV_TILE + 1, 1, z0 + NAV_TILE // 2)]


def nav_goal_sides(solid, call, tile, goals):
    """From navmodel alone, with each of the two goals on its own: (nodes of the tile's own 16 x 16 columns that are nearer to the OUTSIDE goal, of
    them nodes above the floor -- slab nodes --, nodes outside those columns that are nearer to the INSIDE goal).  With both goals in one build the
    first take their distance from beyond the tile's edge, through the halo, and the last from inside it."""
    import navmodel

    dims = solid.shape
    steps = [navmodel.analyse(solid, *call[:6], [g], 0)[0] for g in goals]
    own = (steps[0]["cell"] == np.indices(dims).transpose(1, 2, 3, 0)).all(axis=3)  # the positions that are stand cells: one per node
    d_in, d_out = (np.where(own & (s["distance"] >= 0), s["distance"], np.iinfo(np.int32).max) for s in steps)
    x0, z0 = call[0][0] + tile[0] * NAV_TILE, call[0][2] + tile[1] * NAV_TILE
    in_tile = np.zeros(dims, dtype=bool)
    in_tile[x0:x0 + NAV_TILE, :, z0:z0 + NAV_TILE] = True
    entering = own & in_tile & (d_out < d_in)
    return int(entering.sum()), int(entering[:, 2:, :].sum()), int((own & ~in_tile & (d_in < d_out)).sum())


NAV_CORRIDOR_TILE = (2, 2)
NAV_CORRIDOR_RULE = (1, 1, 0, 0, 0)  # one voxel wide and high, no step up or down: nothing but the corridor is reached


def nav_tile_corridor(slab_columns=0):
    """A corridor one voxel wide and high under rock two voxels thick, inside ONE nav tile (NAV_CORRIDOR_TILE of the whole-world grid): eight rows of
    16 along z at even local x, joined at alternating ends by one cell at the odd x between them: 8 * 16 + 7 = 135 cells, the goal at the first.
    slab_columns: so many wall columns (odd local x, interior z) carry a full stack of slabs above the rock -- nodes nothing reaches, which lift
    the tile's total.  -> (solid, the call, the cells in order)."""
    solid = _floor(NAV_DIMS)
    x0, z0 = NAV_CORRIDOR_TILE[0] * NAV_TILE, NAV_CORRIDOR_TILE[1] * NAV_TILE
    solid[x0 - 3:x0 + NAV_TILE + 3, 1:3, z0 - 3:z0 + NAV_TILE + 3] = True
    cells = []
    for k in range(8):
        zs = range(z0, z0 + NAV_TILE) if k % 2 == 0 else range(z0 + NAV_TILE - 1, z0 - 1, -1)
        cells.extend((x0 + 2 * k, 1, z) for z in zs)
        if k < 7:
            cells.append((x0 + 2 * k + 1, 1, cells[-1][2]))
    c = np.array(cells)
    solid[c[:, 0], c[:, 1], c[:, 2]] = False
    walls = [(x0 + lx, z0 + lz) for lx in range(1, NAV_TILE - 1, 2) for lz in range(1, NAV_TILE - 1)]
    _stack_slabs(solid, walls[:slab_columns], slab_columns * ((NAV_DIMS[1] - 3) // 2), base=2)
    return solid, ((0, 0, 0), NAV_DIMS) + NAV_CORRIDOR_RULE, cells


def nav_corridor_row_sweeps(solid, call, cells):
    """The sweeps the tile corridor needs at the least: its rows along z lie in one tile row each (16 consecutive threads of nav_relax_kernel, one
    wave), every column of a row holds the corridor cell as its SECOND node from the top (after the rock's top), and a wave relaxes equal node
    positions of its columns in one trip: one hop per sweep along a row, 15 hops a row."""
    counts, _ = nav_column_nodes(solid, call)
    rows = {}
    for x, y, z in cells:
        rows.setdefault(x, []).append(z)
    full = [x for x, zs in rows.items() if len(zs) == NAV_TILE]
    assert len(full) == 8 and all(x % 2 == 0 and sorted(rows[x]) == list(range(min(rows[x]), min(rows[x]) + NAV_TILE)) and min(rows[x]) % NAV_TILE == 0 for x in full)
    assert all(counts[x, z] == 2 and solid[x, 2, z] and not solid[x, 3:, z].any() for x in full for z in rows[x]), "rock top first, the corridor cell second"
    return len(full) * (NAV_TILE - 1)


# ---- nav: the widest and the tallest body ----------------------------------------------------------------------------------------------------------------

NAV_WIDE_DIMS = (64, 128, 32)
NAV_WIDE_WALL = 30  # the wall's x
# (z0, z1, clear voxels above the floor) of the wall's openings: 8 wide and 64 clear, 7 wide and 64 clear, 8 wide and 63 clear
NAV_WIDE_OPENINGS = ((1, 9, 64), (13, 20, 64), (23, 31, 63))
NAV_WIDE_GOAL = (52, 9, 12)
# (width, height, stepUp, maxDrop): kNavMaxWidth x kNavMaxHeight, one less of either, and width 5
NAV_WIDE_RULES = ((8, 64, 1, 3), (8, 63, 1, 3), (7, 64, 1, 3), (5, 64, 2, 4), (5, 1, 0, 0))


def nav_wide_world():
    """A floor, a wall across the world at x = NAV_WIDE_WALL up to y = 100 with the openings of NAV_WIDE_OPENINGS (a lintel closes each above its
    clear height), and beyond it two steps one voxel high each, across the whole z."""
    solid = _floor(NAV_WIDE_DIMS)
    solid[NAV_WIDE_WALL, 1:101, :] = True
    for z0, z1, clear in NAV_WIDE_OPENINGS:
        solid[NAV_WIDE_WALL, 1:1 + clear, z0:z1] = False
    solid[40:, 1, :] = True
    solid[48:, 2, :] = True
    return solid


def nav_wide_passable(width, height):
    """The openings a body of width x height passes."""
    return [k for k, (z0, z1, clear) in enumerate(NAV_WIDE_OPENINGS) if z1 - z0 >= width and clear >= height]


def assert_wide_openings(want, width, height):
    """From a field of steps[x, y, z] over nav_wide_world: the wall's openings have a cell exactly where the body fits, and the goal falls onto the
    second step."""
    fits = nav_wide_passable(width, height)
    for k, (z0, _, _) in enumerate(NAV_WIDE_OPENINGS):
        assert (want[NAV_WIDE_WALL, 1, z0]["cell"].tolist() == [NAV_WIDE_WALL, 1, z0]) == (k in fits), (width, height, k)
    assert want[NAV_WIDE_GOAL]["cell"].tolist() == [NAV_WIDE_GOAL[0], 3, NAV_WIDE_GOAL[2]]


# ---- the wave shapes of the component engine, for both rules ---------------------------------------------------------------------------------------------

# name -> (the pieces world, its components in PIECES_BOX, a voxel limit that selects some of them but not all).  The cavity world is the complement.
WAVE_SHAPES = {
    "every wave one root": (lambda: pieces_bars(deep=True), 9, 64),
    "last wave of 1": (lambda: pieces_bars(last=1, deep=True), 9, 64),
    "last wave of 63": (lambda: pieces_bars(last=63, deep=True), 9, 64),
    "every node its own root": (lambda: pieces_checkerboard(deep=True), 2048, 1),
    "lane 0 alone": (pieces_lone_leader, 12, 1),
    "255 listed": (lambda: pieces_checkerboard(255, deep=True), 255, 1),
    "256 listed": (lambda: pieces_checkerboard(256, deep=True), 256, 1),
    "257 listed": (lambda: pieces_checkerboard(257, deep=True), 257, 1),
}


def assert_wave_shape(name, roots):
    """The wave composition a WAVE_SHAPES case is named after, from the roots of its nodes in node order."""
    cut = waves(roots)
    if name == "every wave one root" or name.startswith("last wave of"):
        last = WAVE if name == "every wave one root" else int(name.split()[-1])
        assert len(roots) == 8 * WAVE + last and len(cut[-1]) == last and all(len(set(w)) == 1 for w in cut) and len(set(roots)) == 9
    elif name == "lane 0 alone":
        assert len(roots) == 6 * WAVE
        for w in cut:
            assert len(w) == WAVE and w[0] != w[1] and len(set(w[1:])) == 1
    else:
        count = WAVE_SHAPES[name][1]
        assert len(roots) == count == len(set(roots))


def assert_one_node_in_its_wave(tops, roots, column, lane):
    """The node of `column` is lane `lane` of wave BITS_ROW, and every wave of the box has one root."""
    i = node_at(tops, *column)
    assert (i // WAVE, i % WAVE) == (BITS_ROW, lane) and len(roots) == 9 * WAVE
    assert all(len(w) == WAVE and len(set(w)) == 1 for w in waves(roots)) and len(set(roots)) == 9


# ---- lift: what the waves of the moments and the write kernel hold -----------------------------------------------------------------------------------------

def node_lengths(solid, box_min, box_max):
    """The voxels of every node (a maximal vertical run clipped to the box), in the device's node order."""
    lo, hi = clip(solid.shape, box_min, box_max)
    tops = run_tops(solid, box_min, box_max)
    sub = solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    air = ~sub[tops[:, 0] - lo[0], :, tops[:, 2] - lo[2]]                   # (nodes, Y)
    below = air & (np.arange(sub.shape[1])[None, :] < (tops[:, 1] - lo[1])[:, None])
    # the highest air voxel below the top: the run starts above it (at the box's y0 when there is none)
    start = np.where(below.any(axis=1), sub.shape[1] - np.argmax(below[:, ::-1], axis=1), 0)
    return tops[:, 1] - lo[1] + 1 - start


def node_ranks(solid, box_min, box_max, anchors=0):
    """The place of every node's piece in the list of cvx_world_pieces / cvx_world_lift_pieces (piecesmodel.analyse's order), -1 for a node of an
    anchored piece, in the device's node order."""
    import piecesmodel

    lo, hi = clip(solid.shape, box_min, box_max)
    labels, _ = ndimage.label(solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], structure=SIX)
    floating, _, _ = piecesmodel.analyse(solid, box_min, box_max, anchors)
    rank_of = np.full(int(labels.max()) + 1, -1, dtype=np.int64)
    for k, piece in enumerate(floating):
        s = piece["seed"]
        rank_of[labels[s[0] - lo[0], s[1] - lo[1], s[2] - lo[2]]] = k
    tops = run_tops(solid, box_min, box_max)
    return rank_of[labels[tops[:, 0] - lo[0], tops[:, 1] - lo[1], tops[:, 2] - lo[2]]]


def lift_wave_kinds(ranks, piece_capacity):
    """Per wave of lift_moments_kernel: (path, leader, active lanes).  A lane is active when its node's piece floats and is listed (rank below
    piece_capacity).  path: "idle" (no active lane, the wave returns), "one root" (the active lanes share one piece: one reduction, the leader --
    the FIRST ACTIVE lane -- adds it) or "atomics" (every active lane adds its own sums); leader is None on the other two paths."""
    out = []
    for w in waves(np.asarray(ranks)):
        active = np.flatnonzero((w >= 0) & (w < piece_capacity))
        if len(active) == 0:
            out.append(("idle", None, 0))
        elif len(set(w[active].tolist())) == 1:
            out.append(("one root", int(active[0]), len(active)))
        else:
            out.append(("atomics", None, len(active)))
    return out


def pieces_late_leader(units=4):
    """`units` times two rows of nodes.  The first row (x = 4 u) is a bar `pad` over z = 0 .. 62: 63 nodes.  The second (x = 4 u + 2) is a bar
    `bar` over z = 0 .. 63 at y = 10 with a lone voxel `lone` ABOVE it in column z = 1 (y = 20): 65 nodes in the order bar, lone, bar x 63.  So
    wave 2 u holds pad x 63 and the bar's first node, wave 2 u + 1 the lone voxel on LANE 0 and 63 nodes of the bar.  The list is in seed order
    (first column, there the highest voxel): pad, bar, lone per unit -- the bar's seed lies a wave BEFORE the lone voxel, the only way a piece on
    lane 0 can come later in the list than the piece on the lanes behind it.  With pieceCapacity 3 u + 2 wave 2 u + 1 has lane 0 unlisted and
    lanes 1 .. 63 listed."""
    solid = _floor(PIECES_DIMS)
    for u in range(units):
        solid[4 * u, 30, 0:WAVE - 1] = True
        solid[4 * u + 2, 10, 0:WAVE] = True
        solid[4 * u + 2, 20, 1] = True
    return solid


def pieces_two_roots_apart():
    """Three rows at x = 0, 1, 2.  Row 0 is a bar `a` at y = 10 and row 2 a bar `b` at y = 14, one wave each.  Row 1 holds teeth of `a` (y = 10) on
    the columns z % 3 == 0, teeth of `b` (y = 14) on z % 3 == 1 and lone voxels (y = 20) on z % 3 == 2: wave 1 is a, b, lone, a, b, lone, ...  The
    list is a, b, then the 21 lone voxels: with pieceCapacity 2 the active lanes of wave 1 hold two roots with unlisted nodes between them."""
    solid = _floor(PIECES_DIMS)
    solid[0, 10, :] = True
    solid[2, 14, :] = True
    z = np.arange(WAVE)
    solid[1, 10, z[z % 3 == 0]] = True
    solid[1, 14, z[z % 3 == 1]] = True
    solid[1, 20, z[z % 3 == 2]] = True
    return solid


# sums above 2^32: a pillar of k voxels has moment[1] = (k - 1) k (2 k - 1) / 6 about its lowest voxel, above 2^32 from k = 2345
LIFT_TALL_DIMS = (32, 4096, 32)
LIFT_TALL_BOX = ((0, 1, 0), LIFT_TALL_DIMS)  # above the floor, no anchor bit: everything in the box floats
LIFT_TALL_WALL = 2400


def pillar_moment(k):
    return (k - 1) * k * (2 * k - 1) // 6


def lift_tall_world():
    """A floor and three floating pieces in 32 x 4096 x 32.
    wall    the 64 columns of the rows x = 0 and 1 (the world is 32 columns deep: two rows are the 64 consecutive nodes of wave 0), y 5 .. 2404:
            one piece, 64 nodes of 2400 voxels.
    comb b  in the row x = 4: pillars y 5 .. 2410 on z % 4 == 0, joined by a beam along z at y = 2410.
    comb c  in the same row: pillars y 3 .. 2402 on z % 4 == 2, joined by a beam along z at y = 3.
    Every column of row 4 holds a node of b above a node of c: wave 1 is b, c, b, c, ... with pillars of 2406 and 2400 voxels among them."""
    solid = _floor(LIFT_TALL_DIMS)
    solid[0:2, 5:5 + LIFT_TALL_WALL, :] = True
    z = np.arange(LIFT_TALL_DIMS[2])
    solid[4, 2410, :] = True
    solid[4, 3, :] = True
    for k in z[z % 4 == 0]:
        solid[4, 5:2411, k] = True
    for k in z[z % 4 == 2]:
        solid[4, 3:2403, k] = True
    return solid


def unique_colours(solid):
    """A colour word of its own for every solid voxel of a volume of fewer than 2^24 voxels (alpha 0xFF, the voxel's linear index below it)."""
    assert solid.size <= 1 << 24
    x, y, z = np.nonzero(solid)
    colour = np.zeros(solid.shape, dtype=np.uint32)
    colour[x, y, z] = 0xFF000000 | ((x * solid.shape[1] + y) * solid.shape[2] + z)
    return colour


def brute_sums(solid, box_min, box_max, piece):
    """sum[3] and moment[6] of one listed piece as Python integers, voxel by voxel from the volume: the judge between liftmodel and the kernel."""
    lo, hi = clip(solid.shape, box_min, box_max)
    labels, _ = ndimage.label(solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], structure=SIX)
    s = [int(v) for v in piece["seed"]]
    mn = [int(v) for v in piece["min"]]
    pts = np.argwhere(labels == labels[s[0] - lo[0], s[1] - lo[1], s[2] - lo[2]])
    rel = [[int(p[a]) + lo[a] - mn[a] for p in pts] for a in range(3)]
    sums = [sum(c) for c in rel]
    moments = [sum(v * v for v in c) for c in rel] + [sum(a * b for a, b in zip(rel[i], rel[j])) for i, j in ((0, 1), (1, 2), (2, 0))]
    return sums, moments


# the write kernel: chosen node lengths in node order
LIFT_LENGTH_DIMS = (64, 128, 64)
LIFT_LENGTH_BOX = ((0, 1, 0), LIFT_LENGTH_DIMS)  # with the anchor OUTSIDE: a pillar that stands on the floor (y = 0, outside the box) is anchored
LIFT_LENGTH_BASE = 3                             # the lowest voxel of a floating pillar


def lift_lengths(pattern):
    """A floor and one pillar per entry of `pattern` on the columns (2 i, 2 j), in node order (no two touch: every pillar is a piece).  A positive
    entry is a floating pillar of that many voxels from y = LIFT_LENGTH_BASE; 0 is a pillar of two voxels that stands on the floor -- anchored
    under LIFT_LENGTH_BOX with OUTSIDE, so its node has length 0 in lift_write_kernel's scan.  -> solid"""
    assert len(pattern) <= 32 * 32 and max(pattern) <= LIFT_LENGTH_DIMS[1] - LIFT_LENGTH_BASE
    solid = _floor(LIFT_LENGTH_DIMS)
    for n, length in enumerate(pattern):
        x, z = 2 * (n // 32), 2 * (n % 32)
        if length:
            solid[x, LIFT_LENGTH_BASE:LIFT_LENGTH_BASE + length, z] = True
        else:
            solid[x, 1:3, z] = True
    return solid


def stored_lengths(solid, box_min, box_max, anchors, piece_capacity, voxel_capacity):
    """What lift_write_kernel scans, from the volume and the prefix rule: per node its voxels when its piece is STORED (it floats, is listed, and
    the box volumes of the list up to and including it fit voxel_capacity), else 0."""
    import piecesmodel

    floating, _, _ = piecesmodel.analyse(solid, box_min, box_max, anchors)
    stored, used = 0, 0
    for piece in floating[:piece_capacity]:
        v = int(np.prod(piece["max"].astype(np.int64) - piece["min"]))
        if used + v > voxel_capacity:
            break
        used, stored = used + v, stored + 1
    ranks = node_ranks(solid, box_min, box_max, anchors)
    return np.where((ranks >= 0) & (ranks < stored), node_lengths(solid, box_min, box_max), 0)


_VARIED = [1 + (7 * k + k * k // 5) % 23 for k in range(64)]  # 64 lengths 1 .. 23 with no pattern in the lanes
# name -> (the lengths in node order, the wave totals it is named after)
LIFT_LENGTH_PATTERNS = {
    "lane 0 zero": ([0] + _VARIED[1:], None),
    "lane 63 zero": (_VARIED[:63] + [0], None),
    "lanes 1 to 62 zero": ([7] + [0] * 62 + [9], [16]),
    "63 zeros and 64 on lane 63": ([0] * 63 + [64], [64]),
    "total 64: every lane its own owner": ([1] * 64, [64]),
    "total 65": ([1] * 63 + [2], [65]),
    "total 128": ([3, 1] * 32, [128]),
    "total 4096": ([64] * 64, [4096]),
    "an idle wave between two": (_VARIED + [0] * 64 + [5, 0, 11] * 7, [sum(_VARIED), 0, 112]),
    "three waves and a partial one": ((_VARIED[::-1] + [0, 2, 65, 1]) * 3 + [9] * 5, None),
}


# ---- snapshot: rectangles above 256 workgroups of the diff's count kernel ---------------------------------------------------------------------------------

SNAP_DIMS = (256, 32, 512)
SNAP_GROUP, SNAP_CHUNK = 256, 4096  # the columns of a count workgroup and of a scan chunk
# name -> (x0, z0, sizeX, sizeZ) at levelCount 0, and what the name says: (columns, workgroups, columns of the last workgroup)
SNAP_RECTS = {
    "257 groups, the last partial": ((1, 3, 255, 258), (65790, 257, 254)),
    "257 full groups": ((0, 100, 256, 257), (65792, 257, 256)),
    "256 groups": ((1, 200, 255, 257), (65535, 256, 255)),
    "the whole world": ((0, 0, 256, 512), (131072, 512, 256)),
}
SNAP_ONE_RECT = SNAP_RECTS["257 groups, the last partial"][0]
SNAP_ONE_INDICES = (0, 63, 64, 191, 192, 255, 256, 65535, 65536, 65789)


def snap_terrain():
    """Cheap terrain over SNAP_DIMS: every column solid from y = 0 up to a height of 5 .. 19 (no two neighbours alike)."""
    x, z = np.arange(SNAP_DIMS[0])[:, None], np.arange(SNAP_DIMS[2])[None, :]
    height = 5 + (3 * x + 5 * z + (x * z) % 11) % 15
    return np.arange(SNAP_DIMS[1])[None, :, None] < height[:, None, :]


def snap_counts(rect):
    """(columns, workgroups of the count kernel, columns of its last workgroup, scan chunks) of a rectangle."""
    n = rect[2] * rect[3]
    groups = -(-n // SNAP_GROUP)
    return n, groups, n - (groups - 1) * SNAP_GROUP, -(-n // SNAP_CHUNK)


def snap_place(rect, index):
    """Where linear column `index` of the rectangle lies: ((x, z), workgroup, wave of the workgroup, lane)."""
    assert 0 <= index < rect[2] * rect[3]
    return (rect[0] + index // rect[3], rect[1] + index % rect[3]), index // SNAP_GROUP, index % SNAP_GROUP // WAVE, index % WAVE


def snap_scattered(rect):
    """Edit pattern A: per scan chunk of the rectangle its first and its last column, one column in an even workgroup and one in an odd one
    (at lanes that move from chunk to chunk), and the rectangle's last column -> the sorted linear indices."""
    n, _, _, chunks = snap_counts(rect)
    out = {n - 1}
    for c in range(chunks):
        base = c * SNAP_CHUNK
        picks = [base, base + SNAP_CHUNK - 1, base + 2 * (c % 7) * SNAP_GROUP + (37 * c + 1) % SNAP_GROUP, base + (2 * (c % 5) + 3) * SNAP_GROUP + (91 * c + 5) % SNAP_GROUP]
        out.update(i for i in picks if i < n)
    return sorted(out)


def snap_box_pair(rect):
    """Two columns of SNAP_ONE_RECT and the y of the voxel changed in each: the first in workgroup 0 with the smaller x, the larger z and the higher
    voxel, the second in the last (partial) workgroup with the larger x, the smaller z and the lower voxel.  min[0], max[1] and max[2] of the
    box come from the first, max[0], min[1] and min[2] from the second.  -> ((index, y), (index, y))"""
    n = rect[2] * rect[3]
    return (100, 4), (n - rect[3] + 4, 1)  # (the fifth column of the rectangle's last row)
