"""Worlds whose footprint is not square, and the calls made on them (no device needed).

Every kernel that finds a column computes (x << rowShift) + z with rowShift = log2(dimZ >> lod), clips against dimX and dimZ and wraps with maskX /
maskZ in repeat mode; every one of those expressions reads the same on the wrong axis when dimX == dimZ.  Two sizes separate the axes:
  LONG_Z = (32, 64, 256): rowShift 8, dimX 32 -- a row length taken from dimX aliases inside the record table, which shows as wrong bytes;
  LONG_X = (256, 64, 32): rowShift 5, dimX 256 -- the same mistake leaves the table.
Both have 8192 columns, all six LODs and a short side of exactly one levelCount-5 rounding unit.

writer_cases(dims) and reader_cases(dims) give every call of tests/test_gpu_world_oblong.py as lists of (call, arguments) in the form of
tests/test_world_sequences_later_cpu.py; OblongModels runs them on the dense models alone (tests/test_oblong_worlds_cpu.py), where each case must reach past the short side, and
tests/test_gpu_world_oblong.py runs the same lists on a context beside the models.  A case is a list of runs, every run on a fresh upload; a run's
steps below levelCount 5 come last, so that the levels above are the upload's or a full refresh's."""
import functools

import numpy as np

import cavitymodel
import densemodel
import heightsmodel
import lampmodel
import lightmodel
import piecesmodel
import settlemodel
import surfacerectsmodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _box, _brushed, _sphere
from test_world_brush_cpu import _pick_world
from test_world_light_cpu import ALPHA, RGB
from test_world_models_cpu import identity_at, quarter_forward
from test_world_pieces_cpu import GROUND, OUTSIDE
from test_world_sequences_later_cpu import (SPREAD_AIR, SPREAD_SOLID, Models, _argb, _capsule, _hills, _quad, _shell)

LONG_Z = (32, 64, 256)
LONG_X = (256, 64, 32)
SIZES = [LONG_Z, LONG_X]  # LONG_Z first: a swapped axis stays inside the record table there
SEED = 61
FILL, CARVE, PAINT, REPLACE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT, gpu.COPY_REPLACE
TO_SOLID, TO_AIR, SIGNED = gpu.DISTANCE_TO_SOLID, gpu.DISTANCE_TO_AIR, gpu.DISTANCE_SIGNED
X_AND_Z = 0x01 | 0x20  # per-face flags that tell the axes apart: -X and +Z alone


def swap_xz(faces):
    """Per-face bits (-X +X -Y +Y -Z +Z = 1 2 4 8 16 32) with the X and Z pairs exchanged."""
    return (faces & 0x0C) | ((faces & 0x03) << 4) | ((faces >> 4) & 0x03)


def short_side(dims):
    return min(dims[0], dims[2])


def beyond(dims, columns):
    """Does bool[dimX, dimZ] hold a column past the short side along the long axis?"""
    s = short_side(dims)
    return bool(columns[s:, :].any() if dims[0] > dims[2] else columns[:, s:].any())


def rounded(rect, level, dims):
    """The rectangle (x0, z0, sizeX, sizeZ) rounded out to 2^level columns and clipped to the world."""
    k = (1 << level) - 1
    x0, z0 = max(rect[0], 0) & ~k, max(rect[1], 0) & ~k
    x1, z1 = min((rect[0] + rect[2] + k) & ~k, dims[0]), min((rect[1] + rect[3] + k) & ~k, dims[2])
    return x0, z0, x1 - x0, z1 - z0


# ---- the worlds -------------------------------------------------------------------------------------------------------------------------------------

def dense_world(dims):
    """(solid, colour, WorldSet) of the dense world of the pick tests: terrain, floating slabs, many-run columns, a crater, position-hashed colours."""
    return _pick_world(np.random.default_rng(SEED), dims)


def sparse_world(dims):
    """(solid, colour, WorldSet) of a world that keeps its colours column after column (colorShift 2): one deep tower in every block of 4 x 8 columns
    over a floor one voxel thick, so the blocks would cost more than four times the colours -- and seven columns of eight hold a voxel, so that
    almost no column equals its aliased partner (_pick_world's sparse world has 100 towers among 8192 columns: 2.5 % of the pairs differ)."""
    dx, dy, dz = dims
    rng = np.random.default_rng(SEED + 1)
    x, z = np.meshgrid(np.arange(dx), np.arange(dz), indexing="ij")
    solid = np.zeros(dims, dtype=bool)
    solid[:, 0, :] = (x * 5 + z * 2 + 1) % 8 != 0
    for bx in range(0, dx, 4):
        for bz in range(0, dz, 8):
            cx, cz = bx + int(rng.integers(0, 4)), bz + int(rng.integers(0, 8))
            lo = int(rng.integers(0, 12))
            solid[cx, lo:lo + int(rng.integers(30, 52)), cz] = True
    xs, ys, zs = np.nonzero(solid)
    colour = np.zeros(dims, dtype=np.uint32)
    colour[xs, ys, zs] = (0xFF000000 | ((xs * 2654435761 + ys * 40503 + zs * 2246822519) >> 7) & 0xFFFFFF).astype(np.uint32)
    ws = host.WorldSet.from_voxels(dims, xs.astype(np.int32), ys.astype(np.int32), zs.astype(np.int32), colour[xs, ys, zs], threads=2)
    return solid, colour, ws


@functools.lru_cache(maxsize=None)
def volumes(dims, sparse=False):
    """(solid, colour) of a world, built once; nobody writes into them."""
    solid, colour, ws = (sparse_world if sparse else dense_world)(dims)
    ws.close()
    solid.setflags(write=False)
    colour.setflags(write=False)
    return solid, colour


def _columns_differ(solid, colour, xa, za, xb, zb):
    return (solid[xa, :, za] != solid[xb, :, zb]).any(axis=1) | (colour[xa, :, za] != colour[xb, :, zb]).any(axis=1)


def distinct_fractions(solid, colour):
    """(aliased, transposed): of the columns (x, z) whose partner under a row length taken from dimX -- index x * dimX + z mod the columns -- is
    another column, the fraction that differs from it in solidity or colour; and the same for (x, z) against (z, x) inside the square corner."""
    dx, _, dz = solid.shape
    x, z = (a.ravel() for a in np.meshgrid(np.arange(dx), np.arange(dz), indexing="ij"))
    partner = (x * dx + z) % (dx * dz)
    px, pz = partner // dz, partner % dz
    other = (px != x) | (pz != z)
    aliased = _columns_differ(solid, colour, x[other], z[other], px[other], pz[other]).mean()
    s = min(dx, dz)
    corner = (x < s) & (z < s) & (x != z)
    transposed = _columns_differ(solid, colour, x[corner], z[corner], z[corner], x[corner]).mean()
    return float(aliased), float(transposed)


# ---- placements -------------------------------------------------------------------------------------------------------------------------------------

def whole(dims):
    return (0, 0, 0), tuple(dims)


def corner(dims, y0=0, y1=None):
    """A box up to the far corner that is aligned to nothing: from (dimX / 2 + 3, dimZ / 2 + 5); it reaches past the short side on either world."""
    return (dims[0] // 2 + 3, y0, dims[2] // 2 + 5), (dims[0], dims[1] if y1 is None else y1, dims[2])


def overhang(dims, y0=-5, y1=None):
    """A box that sticks out of all four sides by 5 voxels."""
    return (-5, y0, -5), (dims[0] + 5, dims[1] + 5 if y1 is None else y1, dims[2] + 5)


def rect_of(box):
    return box[0][0], box[0][2], box[1][0] - box[0][0], box[1][2] - box[0][2]


def along(dims, u, v):
    """(x, z) of the point u along the long axis and v along the short one."""
    return (u, v) if dims[0] > dims[2] else (v, u)


def _sun(box, target=RGB, **kw):
    args = dict(sun_dir=(3, 4, 1), sun_level=150, sun_range=64, sky_level=80, sky_range=6, floor_level=25)  # |dx| != |dz|
    args.update(kw)
    return lightmodel.params(*box, target=target, **args)


def _mask(shape, salt):
    n = np.arange(int(np.prod(shape))).reshape(shape)
    return (n * 7 + salt) % 5 != 0


def _shells(dims):
    """Four shells of 8^3 with a cavity each: one that the world's far corner cuts, so that its pocket touches the +X and +Z edges; one that the
    +X edge alone cuts; a sealed one inside the corner box and a sealed one at the near end."""
    dx, _, dz = dims
    return [(dx - 7, 40, dz - 7), (dx - 7, 22, dz - 9), (dx // 2 + 4, 42, dz // 2 + 6), (2, 41, 3)]


def shell_steps(dims):
    return [("write_voxels", dict(write=(at, *_shell(8, 40 + k), REPLACE), label=f"shell {k}")) for k, at in enumerate(_shells(dims))]


def _floating(dims):
    """A block that floats over the far corner column, for settle and REMOVE to find there."""
    dx, _, dz = dims
    return ("brush", dict(strokes=[_box(FILL, (dx - 3, 50, dz - 3), (dx, 53, dz), 0xFF778899)], label="a floating block over the far corner"))


def beams(dims):
    """Two floating beams for cvx_world_lift_pieces, each longer along the long axis than the short side is wide: 40 x 3 columns, two voxels high,
    up to the far corner, and 45 x 1 columns, one voxel high, from the near end.  A swapped LiftElement stride or column decode lays their
    voxels out otherwise in the pools."""
    long_side, s = max(dims[0], dims[2]), short_side(dims)
    (ax, az), (bx, bz) = along(dims, long_side - 40, s - 3), along(dims, long_side, s)
    (cx, cz), (ex, ez) = along(dims, 6, 9), along(dims, 51, 10)
    return ("brush", dict(strokes=[_box(FILL, (ax, 56, az), (bx, 58, bz), 0xFF778899), _box(FILL, (cx, 62, cz), (ex, 63, ez), 0xFF998877)], label="two floating beams along the long axis"))


def tower_strokes(dims, count):
    """`count` towers with colours of their own and sphere carves, spread along the long axis (the strokes of the compaction test at these sizes)."""
    rng = np.random.default_rng(64)
    long_side, s = max(dims[0], dims[2]), short_side(dims)
    out = []
    for k in range(count):
        x, z = along(dims, int((k + 0.5) * long_side / count) - 3, int(rng.integers(0, s - 8)))
        if k % 4 == 3:
            out.append(_sphere(CARVE, (x, int(rng.integers(5, 30)), z), int(rng.integers(3, 9))))
        else:
            out.append(_box(FILL, (x, 0, z), (x + int(rng.integers(2, 7)), int(rng.integers(30, 64)), z + int(rng.integers(2, 9))), int(rng.integers(0, 2**32))))
    return out


def relayout_write(dims):
    """A terrain over the whole footprint, every column solid up to 44 .. 56 voxels: more colours than the tails hold."""
    heights, argb, side = _hills((0, 0, 0), (dims[0], dims[2]), 0, 56, 31)
    return ((0, 0, 0), 56, np.clip(heights, 44, 56), argb, side, 0, 0, REPLACE)


def copy_source(dims):
    """A source box of 40 x 10 columns, 40 along the long axis: legal because its long side is measured against the long side of the world."""
    lo = along(dims, 8, 2)
    hi = along(dims, 48, 12)
    return [lo[0], 0, lo[1]], [hi[0], 48, hi[1]]


def copy_rejected(dims):
    """The same source with its sides exchanged: 40 columns along the short axis.  It would fit if the axes were swapped."""
    lo = along(dims, 2, 2)
    hi = along(dims, 12, 42)
    return dict(srcMin=[lo[0], 0, lo[1]], srcMax=[hi[0], 48, hi[1]], dst=[0, 0, 0], transform=0, op=REPLACE, move=0)


def seam_bodies(dims):
    """Boxes pushed across all four edges of the footprint, from either side: in repeat mode they cross both seams."""
    from movemodel import UNIT as U, body
    dx, dy, dz = dims
    out = []
    for k, y in enumerate((20, 36, 50)):
        for size in ((U, U, U), (2 * U + 7, U + 90, U // 2)):
            for step in (3, 40):
                out += [body(((dx - 2) * U + 11, y * U, (5 + 9 * k) * U), size, (step * U, -U // 2, 13)),   # out through +X
                        body((U // 3, y * U, (dz - 7 - 5 * k) * U), size, (-step * U, 0, -29)),            # out through -X
                        body(((4 + 7 * k) * U, y * U, (dz - 2) * U + 50), size, (17, -U // 4, step * U)),  # out through +Z
                        body(((dx - 6 - 3 * k) * U, y * U, U // 2), size, (-5, 0, -step * U)),             # out through -Z
                        body(((dx - 1) * U, y * U, (dz - 1) * U), size, (step * U, -U, step * U), step_up=U)]  # across the far corner
    return out


SEAM_MAX_T = 100.0  # the seam rays' reach: with |direction| below 1.1 they end within 110 voxels of their origin


def tiled(dims, solid, colour):
    """The bounded world that a repeating one equals for the seam rays: (solid, colour) laid out so often that a ray from the middle tile cannot
    leave, and the (x, 0, z) of the middle tile's corner."""
    kx, kz = (2 * int(np.ceil(1.1 * SEAM_MAX_T / d)) + 1 for d in (dims[0], dims[2]))
    return np.tile(solid, (kx, 1, kz)), np.tile(colour, (kx, 1, kz)), np.float32([kx // 2 * dims[0], 0, kz // 2 * dims[2]])


def seam_rays(dims, n=600):
    """Pick rays that leave through each of the four sides at a shallow angle: in repeat mode they re-enter through the opposite one."""
    rng = np.random.default_rng(17)
    dx, dy, dz = dims
    o = np.stack([rng.uniform(0, dx, n), rng.uniform(0.3 * dy, 0.9 * dy, n), rng.uniform(0, dz, n)], 1)
    side = np.arange(n) % 4
    d = np.stack([rng.uniform(-0.3, 0.3, n), -rng.uniform(0.02, 0.25, n), rng.uniform(-0.3, 0.3, n)], 1)
    d[side == 0, 0], d[side == 1, 0], d[side == 2, 2], d[side == 3, 2] = 1.0, -1.0, 1.0, -1.0
    return o.astype(np.float32), d.astype(np.float32), side


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------

WRITERS = ("brush", "shapes", "stamp", "copy", "write_heights", "place_models", "write_voxels", "fill_cavities", "lamps", "set_column",
           "light", "settle", "remove", "edit", "set_columns", "snapshot_restore", "lift_remove")


def writer_cases(dims):
    """name -> the runs of a writing case; every run starts from a fresh upload of the dense world."""
    dx, dy, dz = dims
    C, O, W = corner(dims), overhang(dims), whole(dims)
    c0, c2 = (C[0][0], C[0][2]), (dx - 11, dz - 11)
    model = (_argb((10, 24, 12), 3), _mask((10, 24, 12), 1))  # 10 x 12 x 24 voxels (x, y, z), kept as (x, z, y)
    turned, turned_size = quarter_forward(1, (10, 12, 24), (dx - 24, 8, dz - 10))
    assert turned_size == (24, 12, 10)
    slab = (_argb((dx + 10, dz + 10, 4), 5), _mask((dx + 10, dz + 10, 4), 2))
    src_min, src_max = copy_source(dims)
    turned_at = along(dims, max(dx, dz) - 10, -4)  # a quarter turn lays the 40 columns across the short axis: clipped on both sides, up to the far end
    hills_c = _hills((c0[0], 4, c0[1]), (dx - c0[0], dz - c0[1]), 4, 44, 7)
    hills_w = _hills((0, 0, 0), (dx, dz), 0, 50, 9)
    hills_o = _hills((-5, 3, -5), (dx + 10, dz + 10), 3, 40, 11)
    dense_c = (_argb((dx - c0[0], dz - c0[1], 20), 13), _mask((dx - c0[0], dz - c0[1], 20), 3))
    dense_o = (_argb((dx + 10, dz + 10, 9), 15), _mask((dx + 10, dz + 10, 9), 4))
    far_lamps = [lampmodel.lamp((dx - 3, 30, dz // 2), 9, 255), lampmodel.lamp((dx // 2, 28, dz - 3), 8, 220), lampmodel.lamp((dx - 2, 40, dz - 2), 10, 240)]
    shells = _shells(dims)
    around = lambda at: ((at[0] - 1, at[1] - 2, at[2] - 1), (at[0] + 9, at[1] + 10, at[2] + 9))  # noqa: E731
    floating = _floating(dims)
    far = (dx - 32, dz - 32, 32, 32)
    cases = {
        "brush": [
            [("brush", dict(strokes=[_sphere(CARVE, (dx - 6, 20, dz - 6), 5)], level_count=0, label="a sphere carve at the far corner"))],
            [("brush", dict(strokes=[_box(PAINT, *C, 0xFF00C0FF)], level_count=2, label="a box paint up to the far corner"))],
            [("brush", dict(strokes=[_box(FILL, (0, 50, 0), (dx, 52, dz), 0xFF2040F0)], label="a box fill over the whole footprint")),
             ("shapes", dict(strokes=[_capsule(FILL, (5, 30, 6), (dx - 6, 36, dz - 5), 3, 0xFF8040C0)], label="a capsule along the long axis")),
             ("brush", dict(strokes=[_box(CARVE, O[0], (O[1][0], 8, O[1][2]))], label="a box carve that overhangs all four sides"))],
        ],
        "stamp": [
            [("stamp", dict(mesh=_quad((c0[0] + 0.5, 30, c0[1] + 0.25), (dx - 0.25, 44, dz - 0.5), 1), op=FILL, level_count=0, label="a slab up to the far corner"))],
            [("stamp", dict(mesh=_quad((c0[0] + 0.5, 4, c0[1] + 0.25), (dx - 0.25, 20, dz - 0.5), 2), op=CARVE, level_count=2, label="a carving slab up to the far corner"))],
            [("stamp", dict(mesh=_quad((0.5, 22, 0.5), (dx - 0.5, 40, dz - 0.5), 3), op=FILL, label="a slab across the long axis")),
             ("stamp", dict(mesh=_quad((-5, 46, -5), (dx + 5, 58, dz + 5), 4), op=FILL, label="a slab that overhangs all four sides"))],
        ],
        "copy": [
            [("copy", dict(placements=[dict(srcMin=src_min, srcMax=src_max, dst=[dx - 6, 6, dz - 7], transform=0, op=REPLACE, move=0)], level_count=0,
                           label="a copy to the far corner, clipped by both edges"))],
            [("copy", dict(placements=[dict(srcMin=src_min, srcMax=src_max, dst=[c0[0], 3, c0[1]], transform=2, op=FILL, move=0)], level_count=2,
                           label="a half turn into the corner box"))],
            [("copy", dict(placements=[dict(srcMin=src_min, srcMax=src_max, dst=[-5, 10, -5], transform=3, op=PAINT, move=1)], label="a moving copy that overhangs the near corner")),
             ("copy", dict(placements=[dict(srcMin=src_min, srcMax=src_max, dst=[turned_at[0], 2, turned_at[1]], transform=1,
                                            op=REPLACE, move=0)], label="a quarter turn: 40 columns along the short axis"))],
        ],
        "write_voxels": [
            [("write_voxels", dict(write=((c0[0], 5, c0[1]), *dense_c, REPLACE), level_count=0, label="a dense box up to the far corner"))],
            [("write_voxels", dict(write=((c0[0], 30, c0[1]), None, dense_c[1], CARVE), level_count=2, label="a carving mask up to the far corner"))],
            [("write_voxels", dict(write=((0, 44, 0), _argb((dx, dz, 6), 17), None, FILL), label="a dense box over the whole footprint")),
             ("write_voxels", dict(write=((-5, -5, -5), *dense_o, REPLACE), label="a dense box that overhangs all four sides"))],
        ],
        "write_heights": [
            [("write_heights", dict(write=((c0[0], 4, c0[1]), 44, *hills_c, 2, heightsmodel.WALLED, REPLACE), level_count=0, label="heights up to the far corner"))],
            [("write_heights", dict(write=((c0[0], 4, c0[1]), 44, *hills_c, 0, 0, FILL), level_count=2, label="heights filled up to the far corner"))],
            [("write_heights", dict(write=((0, 0, 0), 50, *hills_w, 3, 0, REPLACE), label="heights over the whole footprint")),
             ("write_heights", dict(write=((-5, 3, -5), 40, *hills_o, 2, 0, PAINT), label="heights that overhang all four sides"))],
        ],
        "place_models": [
            [("place_models", dict(models=[model], instances=[gpu.model_instance(turned, (10, 12, 24), 0, REPLACE)], level_count=0,
                                   label="a model turned 90 degrees about Y at the far corner"))],
            [("place_models", dict(models=[model], instances=[identity_at((dx - 10, 30, dz - 24), (10, 12, 24), 0, FILL), gpu.model_instance(turned, (10, 12, 24), 0, CARVE)],
                                   level_count=2, label="the model as it lies and turned, at the far corner"))],
            [("place_models", dict(models=[slab, model], instances=[identity_at((-5, 50, -5), (dx + 10, 4, dz + 10), 0, FILL), gpu.model_instance(turned, (10, 12, 24), 1, REPLACE)],
                                   label="a slab that overhangs all four sides and the turned model"))],
        ],
        "light": [
            [("light", dict(p=_sun(C), level_count=0, label="light up to the far corner"))],
            [("light", dict(p=_sun(C, ALPHA, sun_dir=(-2, 5, -7)), level_count=2, label="light to alpha up to the far corner"))],
            [("light", dict(p=_sun(W, sun_dir=(5, 3, -1)), label="light over the whole footprint")),
             ("light", dict(p=_sun(O, ALPHA, sun_dir=(-1, 2, 6), sky_range=3), label="light over a box that overhangs all four sides"))],
        ],
        "lamps": [
            [("lamps", dict(p=_sun(C, sun_level=0, sun_range=0), lamps=far_lamps, level_count=0, label="lamps near both far edges"))],
            [("lamps", dict(p=_sun(C, ALPHA), lamps=far_lamps[::-1], level_count=2, label="lamps and a sun up to the far corner"))],
            [("lamps", dict(p=_sun(O, sun_dir=(-4, 3, 1), sun_range=24), lamps=far_lamps + [lampmodel.lamp((1, 25, 2), 9, 200)], label="lamps over a box that overhangs all four sides"))],
        ],
        "settle": [
            [floating, ("settle", dict(box=C, anchors=GROUND, max_drop=3, level_count=0, label="settle by three up to the far corner"))],
            [floating, ("settle", dict(box=C, anchors=GROUND | OUTSIDE, level_count=2, label="settle up to the far corner"))],
            [floating, ("settle", dict(box=O, anchors=GROUND, label="settle in a box that overhangs all four sides"))],
        ],
        "remove": [
            [floating, ("remove", dict(box=C, anchors=GROUND, level_count=0, label="pieces REMOVE up to the far corner"))],
            [floating, ("remove", dict(box=(C[0], (dx, 56, dz)), anchors=GROUND | OUTSIDE, level_count=2, label="pieces REMOVE below y = 56 up to the far corner"))],
            [floating, ("remove", dict(box=O, anchors=GROUND, label="pieces REMOVE in a box that overhangs all four sides"))],
        ],
        "fill_cavities": [
            shell_steps(dims) + [("fill_cavities", dict(box=around(shells[1]), open_faces=X_AND_Z, level_count=0, label="cavities FILL of the pocket at the +X edge, +X closed"))],
            shell_steps(dims) + [("fill_cavities", dict(box=C, open_faces=0, max_voxels=300, level_count=2, label="cavities FILL up to the far corner, no face open"))],
            shell_steps(dims) + [("fill_cavities", dict(box=((-5, 36, -5), (dx + 5, 56, dz + 5)), open_faces=0x3F, max_voxels=300,
                                                         label="cavities FILL in a box that overhangs all four sides"))],
        ],
        "edit": [
            [("edit", dict(rect=(dx - 13, dz - 11, 13, 11), strokes=[_box(FILL, (dx - 9, 0, dz - 8), (dx - 2, 60, dz), 0xFF102030), _sphere(CARVE, (dx - 5, 20, dz - 5), 4)],
                           level_count=0, label="an edit of 13 x 11 columns at the far corner"))],
            [("edit", dict(rect=(dx - 12, dz - 8, 12, 8), strokes=[_box(FILL, (dx - 12, 40, dz - 8), (dx, 44, dz), 0xFF405060)], level_count=2,
                           label="an edit of 12 x 8 columns at the far corner"))],
            [("edit", dict(rect=far, strokes=[_sphere(CARVE, (dx - 16, 14, dz - 16), 12), _box(FILL, (dx - 30, 0, dz - 5), (dx - 27, 62, dz), 0xFF708090)],
                           label="an edit of the far 32 x 32 columns"))],
        ],
        "set_columns": [
            [("set_columns", dict(rect=far, strokes=[_sphere(CARVE, (dx - 14, 12, dz - 18), 11), _box(FILL, (dx - 4, 0, dz - 31), (dx, 61, dz - 27), 0xFFA0B0C0),
                                                      _box(FILL, (dx - 2, 30, dz - 2), (dx, 40, dz), 0xFFC0B0A0)],
                                  label="set_columns of the far 32 x 32 columns, level by level"))],
        ],
        "snapshot_restore": [
            [("snapshot_restore", dict(rect=rect_of(C), strokes=[_box(FILL, (C[0][0], 20, C[0][2]), (dx, 40, dz), 0xFF2040F0)], level_count=0,
                                       label="a snapshot up to the far corner, levelCount 0"))],
            [("snapshot_restore", dict(rect=rect_of(C), strokes=[_box(CARVE, (C[0][0], 0, C[0][2]), (dx, 12, dz))], level_count=2,
                                       label="a snapshot up to the far corner, levelCount 2"))],
            [("snapshot_restore", dict(rect=rect_of(O), strokes=[_box(PAINT, *W, 0xFF00C0FF), _sphere(CARVE, (dx - 6, 20, dz - 6), 9)], level_count=5,
                                       label="a snapshot of a rectangle that overhangs all four sides"))],
        ],
        "lift_remove": [
            # (boxes from y = 52: they cut the terrain's columns, whose tops float there with nothing at y = 0 to hold them, and hold a quarter of the
            # world's single floating voxels)
            [beams(dims), ("lift_remove", dict(box=corner(dims, 52), anchors=GROUND, level_count=0, label="lift REMOVE up to the far corner"))],
            [beams(dims), ("lift_remove", dict(box=corner(dims, 52, 60), anchors=GROUND | OUTSIDE, level_count=2, label="lift REMOVE below y = 60 up to the far corner"))],
            [beams(dims), ("lift_remove", dict(box=overhang(dims, 52), anchors=GROUND, label="lift REMOVE in a box that overhangs all four sides"))],
        ],
        "rounds to the short side": [
            [("brush", dict(strokes=[_box(FILL, (dx - 3, 20, dz - 3), (dx, 30, dz), 0xFF00FF00)], label="three columns at the far corner, levelCount 5"))],
        ],
    }
    return cases


NEEDS_SHELLS = ("report_cavities", "lift_copy")  # the reading cases that begin with writes: the dense world encloses no cavity and floats no long piece


def reader_cases(dims):
    """name -> the steps of a reading case, all on one upload of the dense world that nothing writes into (NEEDS_SHELLS: on an upload of their own)."""
    dx, dy, dz = dims
    C, O, W = corner(dims), overhang(dims), whole(dims)
    ends = [along(dims, 2, 3), along(dims, max(dx, dz) - 3, short_side(dims) - 4)]  # both ends of the long axis
    goals = [(x, 60, z) for x, z in ends]
    three = lambda call, name, **kw: [(call, dict(box=box, label=f"{name}, {where}", **kw))  # noqa: E731
                                      for where, box in (("the whole footprint", W), ("up to the far corner", C), ("overhanging all four sides", O))]
    cases = {
        "read_voxels": three("read_voxels", "read_voxels"),
        "read_heights": three("read_heights", "read_heights"),
        "read_model": [("read_model", dict(src_min=(dx - 10, 16, dz - 24), size=(10, 16, 24), transform=1, label="read_model of the far corner, turned 90 degrees about Y")),
                       ("read_model", dict(src_min=(dx - 10, 16, dz - 24), size=(10, 16, 24), transform=0, label="read_model of the far corner, as it lies"))],
        "surface": three("surface", "surface", solid_outside=X_AND_Z),
        "surface_rects": three("surface_rects", "surface_rects", solid_outside=X_AND_Z),
        "distance": [step for mode in (TO_SOLID, TO_AIR, SIGNED) for step in three("distance", f"distance mode {mode}", mode=mode, solid_outside=X_AND_Z)],
        "spread": [("spread", dict(box=W, seeds=goals, medium=SPREAD_AIR, max_steps=400, label="spread through the air from both ends of the long axis")),
                   ("spread", dict(box=C, seeds=[(dx - 2, 60, dz - 2)], medium=SPREAD_AIR, step_faces=0x3F & ~X_AND_Z, max_steps=400, label="spread without -X and +Z steps up to the far corner")),
                   ("spread", dict(box=O, seeds=[(x, 1, z) for x, z in ends], medium=SPREAD_SOLID, step_faces=0x3F & ~swap_xz(X_AND_Z), max_steps=400,
                                   label="spread through the solid in a box that overhangs all four sides"))],
        "nav": [("nav", dict(call=(*W, 1, 2, 1, 3, 0), goals=goals, label="nav over the whole footprint, goals at both ends")),
                ("nav", dict(call=(*C, 2, 2, 1, 3, 0), goals=[(dx - 3, 60, dz - 3)], label="nav up to the far corner, two voxels wide")),
                ("nav", dict(call=(*O, 1, 3, 1, 2, 0), goals=goals[::-1], label="nav in a box that overhangs all four sides"))],
        "report_pieces": three("report_pieces", "pieces REPORT", anchors=GROUND),
        "report_cavities": shell_steps(dims) + three("report_cavities", "cavities REPORT", open_faces=X_AND_Z),
        "lift_copy": [beams(dims)] + [("lift_copy", dict(box=box, anchors=GROUND, label=f"lift COPY, {where}"))
                                       for where, box in (("the whole footprint from y = 52", ((0, 52, 0), tuple(dims))), ("up to the far corner", corner(dims, 52)),
                                                          ("overhanging all four sides", overhang(dims, 52)))],
    }
    return cases


# ---- the models -------------------------------------------------------------------------------------------------------------------------------------

class OblongModels(Models):
    """Models with the calls the newer sequences do not run, and a record of where every step reaches: `written` (bool[dimX, dimZ]) holds the
    columns the writers changed, `seen` the columns in which a reader's expected result is not trivial.  quick: leave out the second run of a model
    with the X and Z bits of the call's flags exchanged (the GPU test, which runs the same lists)."""
    quick = False

    def __init__(self, dims, solid, colour, work):
        self.dims, self.solid, self.colour, self.work, self.last, self.before, self.steps = dims, solid, colour, work, None, None, 0
        self.written = np.zeros((dims[0], dims[2]), dtype=bool)
        self.seen = np.zeros((dims[0], dims[2]), dtype=bool)

    def run(self, plan):
        for call, args in plan:
            args = {k: v for k, v in args.items() if k not in ("level_count", "check")}
            out = getattr(self, "m_" + call)(**args)
            if call in WRITERS:
                self.solid, self.colour = out
            self.steps += 1

    def changed(self, after, label, overlaps=False):
        after = super().changed(after, label, overlaps)
        self.written |= self.last
        return after

    def see(self, xs, zs):
        """Columns (world coordinates, any integers) in which a reader returns something."""
        xs, zs = np.asarray(xs).ravel(), np.asarray(zs).ravel()
        ok = (xs >= 0) & (xs < self.dims[0]) & (zs >= 0) & (zs < self.dims[2])
        self.seen[xs[ok], zs[ok]] = True

    def see_field(self, mask, origin):
        """mask: bool (X, Z, Y) or (X, Z) whose element [0, 0] is the column `origin` = (x, z)."""
        i, k = np.nonzero(mask.reshape(mask.shape[0], mask.shape[1], -1).any(axis=2))
        self.see(i + origin[0], k + origin[1])

    def see_boxes(self, records):
        for r in records:
            x, z = np.meshgrid(np.arange(r["min"][0], r["max"][0]), np.arange(r["min"][2], r["max"][2]), indexing="ij")
            self.see(x, z)

    def flags_matter(self, call, want, swapped, label):
        a, b = (want[0] if isinstance(want, tuple) else want), (swapped[0] if isinstance(swapped, tuple) else swapped)
        assert a.shape != b.shape or a.tobytes() != b.tobytes(), f"{label}: {call} gives the same with the X and Z bits of its flags exchanged"

    # -- writers ----------------------------------------------------------------------------------------------------------------------------------
    def m_light(self, p, label, **_):
        mask, _ = lightmodel.shades(self.solid, p)
        assert mask.any(), f"{label}: the box holds no voxel"
        assert abs(p["sun_dir"][0]) != abs(p["sun_dir"][2])
        return self.changed((self.solid, lightmodel.light(self.solid, self.colour, p)), label)

    def m_settle(self, box, anchors, label, max_drop=0, **_):
        want, drops, summary, after = settlemodel.settle(self.solid, self.colour, *box, anchors, max_drop)
        assert summary["fallenPieces"] > 0, f"{label}: nothing falls"
        return self.changed(after, label)

    def m_remove(self, box, anchors, label, **_):
        want, summary, _ = piecesmodel.analyse(self.solid, *box, anchors)
        assert summary["floatingPieces"] > 0, f"{label}: nothing floats"
        return self.changed(piecesmodel.remove(self.solid, self.colour, *box, anchors), label)

    def long_pieces(self, lift, label):
        """The stored pieces of a lift that are longer along the long axis than the short side: there must be one, past the short side."""
        axis = 0 if self.dims[0] > self.dims[2] else 2
        stored = lift.pieces["piece"][:lift.summary["storedPieces"]]
        long = [p for p in stored if int(p["max"][axis]) - int(p["min"][axis]) > short_side(self.dims)]
        cols = np.zeros((self.dims[0], self.dims[2]), dtype=bool)
        for p in long:
            cols[p["min"][0]:p["max"][0], p["min"][2]:p["max"][2]] = True
        assert long and beyond(self.dims, cols), f"{label}: no stored piece is longer than the short side and reaches past it"
        return stored

    def m_lift_remove(self, box, anchors, label, **kw):
        after = super().m_lift_remove(box, anchors, label, **kw)
        self.long_pieces(self.lift[0], label)
        return after

    def m_fill_cavities(self, box, label, open_faces=0x3F, max_voxels=0, argb=0xFF123456, overlaps=False, **_):
        after = super().m_fill_cavities(box, label, open_faces, max_voxels, argb, overlaps)
        if open_faces not in (0, 0x3F) and not self.quick:
            assert swap_xz(open_faces) != open_faces
            other = cavitymodel.fill(self.solid, self.colour, *box, swap_xz(open_faces), max_voxels, argb)
            assert (other[0] != after[0]).any(), f"{label}: the same cavities with the X and Z bits of openFaces exchanged"
        return after

    def m_edit(self, rect, strokes, label, **_):
        """The columns of `rect` replaced by those of the world the strokes make: the strokes must stay inside it."""
        after = self.changed(_brushed(self.solid, self.colour, strokes), label)
        x0, z0, sx, sz = rect
        inside = np.zeros_like(self.last)
        inside[x0:x0 + sx, z0:z0 + sz] = True
        assert not (self.last & ~inside).any(), f"{label}: the strokes change columns outside {rect}"
        return after

    m_set_columns = m_edit

    def m_snapshot_restore(self, rect, strokes, label, level_count=5, **_):
        """Snapshot, strokes, restore: the volume is as before; the strokes count as what the case writes."""
        state, before = (self.solid, self.colour), self.before
        self.changed(_brushed(self.solid, self.colour, strokes), label)
        x0, z0, sx, sz = rounded(rect, 0, self.dims)
        held = np.zeros_like(self.last)
        held[x0:x0 + sx, z0:z0 + sz] = True
        assert not (self.last & ~held).any(), f"{label}: the strokes change columns outside the snapshot"
        self.before = before
        return state

    # -- readers ----------------------------------------------------------------------------------------------------------------------------------
    def m_read_voxels(self, box, label, holds=None):
        want = super().m_read_voxels(box, label, holds)
        self.see_field(want[1], (box[0][0], box[0][2]))
        return want

    def m_read_heights(self, box, label, holds=None):
        want = super().m_read_heights(box, label, holds)
        self.see_field(want[1] != 0, (box[0][0], box[0][2]))
        return want

    def m_read_model(self, src_min, size, transform, label, holds=None):
        want = super().m_read_model(src_min, size, transform, label, holds)
        dense = densemodel.read(self.solid, self.colour, (src_min, tuple(src_min[i] + size[i] for i in range(3))))
        self.see_field(dense[1], (src_min[0], src_min[2]))
        return want

    def m_surface(self, box, label, solid_outside=0x04, flags=0, holds=None):
        want = super().m_surface(box, label, solid_outside, flags, holds)
        self.see(want[0]["voxel"][:, 0], want[0]["voxel"][:, 2])
        if solid_outside & 0x33 and not self.quick:
            import surfacemodel
            self.flags_matter("surface", want, surfacemodel.surface(self.solid, self.colour, *box, swap_xz(solid_outside), flags), label)
        return want

    def m_surface_rects(self, box, label, solid_outside=0x04, flags=0, holds=None):
        want = surfacerectsmodel.rects(self.solid, self.colour, *box, solid_outside, flags)
        assert len(want[0]) > 0, label
        self.see(want[0]["voxel"][:, 0], want[0]["voxel"][:, 2])
        if solid_outside & 0x33 and not self.quick:
            self.flags_matter("surface_rects", want, surfacerectsmodel.rects(self.solid, self.colour, *box, swap_xz(solid_outside), flags), label)
        return self.held(want, holds, label)

    def m_distance(self, box, label, R=8, mode=TO_SOLID, solid_outside=0x04, holds=None):
        import distancemodel
        want = super().m_distance(box, label, R, mode, solid_outside, holds)
        self.see_field((want != 0) & (abs(want) != distancemodel.FAR), (box[0][0], box[0][2]))
        if solid_outside & 0x33 and not self.quick:
            self.flags_matter("distance", want, distancemodel.field(self.solid, box, R, mode, swap_xz(solid_outside)), label)
        return want

    def m_spread(self, box, seeds, medium, label, step_faces=0x3F, max_steps=200, holds=None):
        import spreadmodel
        want = super().m_spread(box, seeds, medium, label, step_faces, max_steps, holds)
        assert want[0].shape == (box[1][0] - box[0][0], box[1][2] - box[0][2], box[1][1] - box[0][1])  # (spreadmodel.passable: the box as given, unclipped)
        self.see_field(want[0] > 0, (box[0][0], box[0][2]))
        if step_faces != 0x3F and not self.quick:
            self.flags_matter("spread", want, spreadmodel.field(self.solid, *box, seeds, medium, swap_xz(step_faces), max_steps), label)
        return want

    def m_nav(self, call, goals, label, holds=None):
        want = super().m_nav(call, goals, label, holds)
        steps = want[0].reshape(-1)
        reached = steps[steps["distance"] > 0]
        self.see(reached["cell"][:, 0], reached["cell"][:, 2])
        return want

    def m_lift_copy(self, box, anchors, label, capacity=8192, voxel_capacity=None, holds=None):
        want = super().m_lift_copy(box, anchors, label, capacity, voxel_capacity, holds)
        self.see_boxes(self.long_pieces(want[0], label))
        return want

    def m_report_pieces(self, box, anchors, label, holds=None):
        want, summary, _ = piecesmodel.analyse(self.solid, *box, anchors)
        assert summary["floatingPieces"] > 0, label
        self.see_boxes(want)
        return self.held((want, summary), holds, label)

    def m_report_cavities(self, box, label, open_faces=0x3F, max_voxels=0, holds=None):
        want = super().m_report_cavities(box, label, open_faces, max_voxels, holds)
        assert len(want[0]) > 0, f"{label}: the model selects no cavity"
        self.see_boxes(want[0])
        if open_faces not in (0, 0x3F) and not self.quick:
            other = cavitymodel.analyse(self.solid, *box, swap_xz(open_faces), max_voxels)
            self.flags_matter("cavities", want, (other[0], other[1]), label)
        return want
