"""GPU: cvx_world_stamp_mesh at the limits of the kernels that exist only on the device (cpuvox_amd/csrc/cvx_stamp.hip, steps 1 to 6).

The enumeration of (triangle, column) pairs with its binary search, the per-triangle cap, emit, the radix sort, the merge of duplicates and the
bounding box are not in cvx_stamp.h, so the host build of the rules (tests/stamp_rules.cpp) cannot reach them.  Every case here builds a mesh
whose counts put one of those steps at an edge: the number of kept hits n around the sort's waves, rounds and tiles (transparent hits among them
or not), n on both sides of the number of pairs (which list buffers step 6 uses), a cap that falls inside a column of a triangle that is not the
first, runs of 300 equal keys, stamps that leave through each early exit, blocks and scan chunks of triangles without columns, a box of two
corners, slivers, and a column the format cannot hold.

Each case asserts the counts it is named after FROM THE HOST (stampmodel.counts / hits: TriangleSetup, TriangleHit and TriangleColour in the
host's loop order) before the device is called; only then is the device's world compared with the model: stampmodel.voxelise (the host loop,
triangle after triangle, with the cap), merged in numpy (stampmodel.apply_stamp on a dense volume; stampmodel.merge alone where the world is
empty and too tall for one), rebuilt with host.WorldSet.from_voxels, all six levels byte for byte through read_level.  Nothing has a tolerance."""
import numpy as np
import pytest

import stampmodel
from cpuvox_amd import gpu, host
from test_gpu_world_edit import _colour
from test_world_stamp_cpu import _random_triangles, _slivers

pytestmark = pytest.mark.gpu

FILL, CARVE, PAINT = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT

# The constants the cases are named after (cvx_stamp.hip unless another source is given)
RADIX_BITS = 4                # kRadixBits: bits per sort pass
RADIX_TILE = 256 * 8          # kRadixTile = kRadixThreads * kRadixRounds: the items of one sort block
WAVE = 64                     # CVX_WAVE: the scatter ranks its items by wave ballots
BLOCK = 256                   # threads per block of the pair (count, cap, emit), head and merge kernels
CAP = 262144                  # cvxs::kVoxelizeBufferMax (cvx_stamp.h): hits kept per triangle
SCAN_CHUNK = 256 * 16         # CVX_SCAN_THREADS * CVX_SCAN_PER_THREAD (cvx_context.h): one block of cvxi::ExclusiveScan
assert RADIX_TILE == 2048 and SCAN_CHUNK == 4096

SMALL, WIDE = (64, 64, 64), (128, 64, 128)
TALL = (128, 8192, 128)
WALL = [[10.3, 2, 10.2], [10.9, 60, 50.1], [11.4, 3, 52.7]]        # steep: 138 columns, 1255 hits, up to 45 a column (in WIDE)
FLAT = [[20.3, 10.2, 20.1], [60.7, 10.2, 25.3], [30.2, 10.2, 70.9]]  # one hit a column at most, through the terrain's hills


def _bit_width(v):
    return int(v).bit_length()


def _passes(dims):
    """The sort passes of a world: the host code's keyBits (cvx_world_stamp_mesh, step 4) over the bits of a pass."""
    key_bits = _bit_width(dims[0] * dims[2]) + max(1, _bit_width(dims[1] - 1))
    return -(-key_bits // RADIX_BITS)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("stamp_limits")
    return d, stampmodel.rules(d)


def _terrain(dims):
    """The rolling terrain with floating slabs of tests/test_gpu_world_edit.py for any dims, with blocks of 8 x 8 columns left empty."""
    x, y, z = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    h = 14 + (6 * np.sin(x / 9.0) + 5 * np.cos(z / 7.0)).astype(np.int64)
    solid = y < h
    solid |= (y >= 34) & (y < 38) & ((x // 16 + z // 16) % 3 == 0)
    solid &= (x // 8 + z // 8) % 4 != 1
    return solid


def _dense(solid):
    x, y, z = np.nonzero(solid)
    colour = np.zeros(solid.shape, dtype=np.uint32)
    colour[x, y, z] = _colour(x, y, z)
    return colour


def _world(solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(solid.shape, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=4)


def _empty(dims):
    e = np.zeros(0, dtype=np.int32)
    return host.WorldSet.from_voxels(dims, e, e, e, np.zeros(0, dtype=np.uint32))


@pytest.fixture(scope="module")
def terrains():
    """dims -> (solid, colour, world set): built once, never changed (every case copies the volume and uploads the world for itself)."""
    out = {}
    for dims in (SMALL, WIDE):
        solid = _terrain(dims)
        colour = _dense(solid)
        out[dims] = (solid, colour, _world(solid, colour))
    return out


def _uploaded(ws):
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
    except BaseException:
        ctx.close()
        raise
    return ctx


def _levels(ctx):
    return [ctx.read_level(k)[0] for k in range(6)]


def _assert_levels(ctx, want, label, level_count=5, above=None):
    """Levels 0 .. level_count are `want`'s, the ones above (which the stamp does not rebuild) are `above`'s."""
    for k in range(6):
        ws = want if k <= level_count else above
        assert ctx.read_level(k)[0] == ws.storage(k).tobytes(), f"{label}: LOD {k} differs from the host rebuild of the model"


def _mesh(triangles, rgba=None, textures=(), **more):
    """triangles: [T, 3, 3] corner positions; rgba: [T * 3, 4] or None (white); more: uv, material per vertex."""
    pos = np.asarray(triangles, dtype=np.float32).reshape(-1, 3)
    v = {"position": pos, **more}
    if rgba is not None:
        v["rgba"] = rgba
    return host.Mesh.from_arrays(v, textures=textures)


def _rgba(rng, vertices):
    c = rng.integers(0, 256, size=(vertices, 4)).astype(np.uint8)
    c[:, 3] = 255
    return c


def _one_hit(voxel, e):
    """A right triangle with legs e inside one voxel: exactly one hit (asserted wherever it is used), 4 to 9 box columns."""
    c = np.asarray(voxel, dtype=np.float64) + 0.5
    return [c, c + [e, 0, 0], c + [0, 0, e]]


def _keys(dims, x, y, z):
    return (np.asarray(x, np.int64) * dims[1] + np.asarray(y, np.int64)) * dims[2] + np.asarray(z, np.int64)


def _model(work, terrain, mesh, op):
    """The model's world after stamping `mesh` into the terrain with op: (world set, the emitted voxels)."""
    d, rules = work
    solid, colour, _ = terrain
    x, y, z, argb = stampmodel.voxelise(rules, mesh, solid.shape, d)
    after = stampmodel.apply_stamp(solid.copy(), colour.copy(), x, y, z, argb, op)
    return _world(*after), (x, y, z, argb)


# ---- 1. exact numbers of kept hits: the sort's waves, rounds and tiles ------------------------------------------------------------------------------

HIT_COUNTS = [1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1, 2 * RADIX_TILE - 1, 2 * RADIX_TILE,
              2 * RADIX_TILE + 1]
BALLAST = [[2.3, 5.2, 3.1], [12.6, 24.4, 9.8], [4.2, 9.7, 22.3]]   # an ordinary triangle in x < 15: columns of several hits among the single ones


def _exact_mesh(work, dims, solid, n, transparent=0):
    """A mesh of exactly n kept hits in n distinct voxels: one-hit triangles at x >= 17 (every second column, seven heights: inside the hills,
    in the air above them and in the empty columns), around the ballast triangle from n = 255 on.  transparent: every so-manieth triangle has a
    material whose texels all have alpha 100 (its hits are kept and give no voxel: a sentinel key each)."""
    d, rules = work
    rng = np.random.default_rng(1000 + n)
    ballast = 0
    if n >= BLOCK - 1:
        ballast = int(stampmodel.counts(rules, _mesh([BALLAST]), dims, d)["kept"][0])
        assert 2 * WAVE < ballast < BLOCK - 1, ballast
    xs, ys, zs = np.meshgrid(np.arange(17, dims[0] - 2, 2), [2, 8, 20, 30, 40, 50, 60], np.arange(3, dims[2] - 2, 2), indexing="ij")
    spots = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], axis=1)
    spots = spots[rng.permutation(len(spots))[:n - ballast]]
    assert len(spots) == n - ballast
    triangles = [_one_hit(v, rng.uniform(0.01, 0.3)) for v in spots]
    if ballast:
        triangles.insert(len(triangles) // 2, BALLAST)
    see_through = np.zeros(len(triangles), dtype=bool)
    if transparent:
        see_through[::transparent] = True
    material = np.repeat(np.where(see_through, 0, -1), 3)
    mesh = _mesh(triangles, _rgba(rng, 3 * len(triangles)), [np.full((2, 2, 4), 100, dtype=np.uint8)] if transparent else (), material=material)
    c = stampmodel.counts(rules, mesh, dims, d)
    single = np.ones(len(c), dtype=bool)
    if ballast:
        single[len(spots) // 2] = False
    assert (c["hits"][single] == 1).all() and (c["pairs"][single] >= 4).all() and (c["pairs"][single] <= 9).all()
    assert int(c["kept"].sum()) == n, f"the mesh keeps {int(c['kept'].sum())} hits"
    assert (c["opaque"][see_through] == 0).all() and (c["opaque"][~see_through] == c["kept"][~see_through]).all()
    assert n <= int(c["pairs"].sum())
    if n >= WAVE - 1:
        below = solid[spots[:, 0], spots[:, 1], spots[:, 2]]
        bare = ~solid[spots[:, 0], :, spots[:, 2]].any(axis=1)
        assert below.any() and (~below & ~bare).any() and bare.any(), "hits inside the terrain, in the air above it and in empty columns"
    return mesh


@pytest.mark.parametrize("dims,parity", [(SMALL, 1), (WIDE, 0)])
@pytest.mark.parametrize("n", HIT_COUNTS)
def test_a_stamp_of_exactly_n_kept_hits(work, terrains, n, dims, parity):
    """n kept hits, all of different voxels: one item, a wave / a block's round / a tile / two tiles with one item missing, full, and one over.
    64 x 64 x 64 has keys of 19 bits (5 passes, the sorted keys end in the second buffer), 128 x 64 x 128 of 21 (6 passes, the first)."""
    assert _passes(dims) == (5 if dims == SMALL else 6) and _passes(dims) % 2 == parity
    mesh = _exact_mesh(work, dims, terrains[dims][0], n)
    want, (x, y, z, _) = _model(work, terrains[dims], mesh, FILL)
    assert len(x) == n and len(np.unique(_keys(dims, x, y, z))) == n, "n hits in n voxels"
    ctx = _uploaded(terrains[dims][2])
    try:
        assert ctx.stamp_mesh(mesh, FILL, 5) > 0.0
        _assert_levels(ctx, want, f"{n} hits in {dims}")
    finally:
        ctx.close()
        want.close()


@pytest.mark.parametrize("dims", [SMALL, WIDE])
@pytest.mark.parametrize("n", [RADIX_TILE - 1, RADIX_TILE, RADIX_TILE + 1])
def test_n_kept_hits_with_transparent_ones_among_them(work, terrains, n, dims):
    """The tile's edge again with every third triangle transparent: a third of the n keys are the sentinel, spread through the tile before
    the sort and behind every real key after it; the heads and the merge must pass them over."""
    mesh = _exact_mesh(work, dims, terrains[dims][0], n, transparent=3)
    c = stampmodel.counts(work[1], mesh, dims, work[0])
    sentinels = int((c["kept"] - c["opaque"]).sum())
    assert int(c["kept"].sum()) == n and n // 4 < sentinels < n // 2 and c["opaque"][0] == 0
    want, (x, y, z, _) = _model(work, terrains[dims], mesh, FILL)
    assert len(x) == n - sentinels and len(np.unique(_keys(dims, x, y, z))) == len(x)
    ctx = _uploaded(terrains[dims][2])
    try:
        assert ctx.stamp_mesh(mesh, FILL, 5) > 0.0
        _assert_levels(ctx, want, f"{n} hits, {sentinels} transparent, in {dims}")
    finally:
        ctx.close()
        want.close()


# ---- 2. both branches of the voxel list's buffers ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,op", [("wall", FILL), ("wall", CARVE), ("flat", FILL), ("flat", PAINT)])
def test_the_voxel_list_in_new_buffers_and_in_the_pairs_buffers(work, terrains, name, op):
    """One triangle: the steep wall has more kept hits than pairs (step 6 allocates the voxel list), the flat one fewer (the list goes into the
    pairs' arrays)."""
    d, rules = work
    mesh = _mesh([WALL if name == "wall" else FLAT], [[250, 10, 10, 255], [10, 250, 10, 255], [10, 10, 250, 255]])
    c = stampmodel.counts(rules, mesh, WIDE, d)[0]
    if name == "wall":
        assert (c["pairs"], c["hits"], c["kept"], c["column_max"]) == (138, 1255, 1255, 45) and c["kept"] > c["pairs"]
    else:
        assert 0 < c["kept"] <= c["pairs"] and c["column_max"] == 1
    want, _ = _model(work, terrains[WIDE], mesh, op)
    assert want.storage(0).tobytes() != terrains[WIDE][2].storage(0).tobytes(), "the stamp changes the world"
    ctx = _uploaded(terrains[WIDE][2])
    try:
        assert ctx.stamp_mesh(mesh, op, 5) > 0.0
        _assert_levels(ctx, want, f"{name}, op {op}")
    finally:
        ctx.close()
        want.close()


# ---- 3. the cap behind other triangles and inside a column -------------------------------------------------------------------------------------

def _around(voxel):
    """A small triangle through the middle of `voxel`."""
    c = np.asarray(voxel, dtype=np.float64) + 0.5
    return [c + [-1.2, 0.0, -0.9], c + [1.4, 0.3, -0.2], c + [0.1, -0.2, 1.6]]


def _capped_mesh(work):
    d, rules = work
    f = np.float32
    ramp = np.float32([[0.2, 1.3, 0.4], [127.6, f(1.3) + f(36) * f(127.4), 3.1], [2.7, 9.9, 127.2]])
    t, x, y, z = stampmodel.hits(rules, _mesh([ramp]), TALL, d)
    assert len(t) == 290965 > CAP
    all_keys = _keys(TALL, x, y, z)
    kept, dropped = all_keys[:CAP], all_keys[CAP:]
    assert not np.isin(dropped, kept).any()
    on_kept, on_dropped = 100000, CAP + 15000
    triangles = [_one_hit((5, 100, 5), 0.2), [[9, 9, 9], [9, 9, 9], [12, 40, 30]], ramp,
                 _around((x[on_kept], y[on_kept], z[on_kept])), _around((x[on_dropped], y[on_dropped], z[on_dropped]))]
    rng = np.random.default_rng(33)
    mesh = _mesh(triangles, _rgba(rng, 15))
    c = stampmodel.counts(rules, mesh, TALL, d)
    assert c["hits"][0] == 1 and c["pairs"][1] == 0
    assert (c["pairs"][2], c["hits"][2], c["kept"][2], c["column_max"][2], c["midpair"][2]) == (16384, 290965, CAP, 37, 1)
    assert c["pairs"][:2].sum() > 0, "the capped triangle's first pair is not pair 0"
    t, x, y, z = stampmodel.hits(rules, mesh, TALL, d)
    fourth, last = _keys(TALL, x[t == 3], y[t == 3], z[t == 3]), _keys(TALL, x[t == 4], y[t == 4], z[t == 4])
    assert np.isin(fourth, kept).any(), "the fourth triangle shares voxels with the ramp's kept ones"
    assert np.isin(last, dropped).any() and not np.isin(last, kept).any(), "the last triangle lies on voxels the cap dropped"
    return mesh, last


def test_the_cap_of_a_later_triangle_inside_a_column(work):
    """A small triangle, a triangle without area, then a ramp of 290965 hits over all 16384 columns of an empty 128 x 8192 x 128 world, up to 37
    a column: its rank starts behind the first triangle's pairs and its 262144th hit is in the middle of a column, so cap_kernel cuts a column's
    hits and emit_kernel ends a column early.  Two more triangles follow, one on voxels the ramp kept, one on voxels the cap dropped."""
    d, rules = work
    mesh, last = _capped_mesh(work)
    x, y, z, argb = stampmodel.voxelise(rules, mesh, TALL, d)
    assert len(x) == int(stampmodel.counts(rules, mesh, TALL, d)["kept"].sum())
    ux, uy, uz, merged = stampmodel.merge(x, y, z, argb)
    assert np.isin(last, _keys(TALL, ux, uy, uz)).all(), "the last triangle's voxels are all in the model"
    want = host.WorldSet.from_voxels(TALL, ux, uy, uz, merged, threads=4)
    empty = _empty(TALL)
    ctx = _uploaded(empty)
    try:
        assert ctx.stamp_mesh(mesh, FILL, 5) > 0.0
        _assert_levels(ctx, want, "the capped ramp")
    finally:
        ctx.close()
        want.close()
        empty.close()


# ---- 4. long runs of duplicates ------------------------------------------------------------------------------------------------------------------

COPIES = 300


@pytest.mark.parametrize("textured", [False, True])
def test_runs_of_300_equal_keys(work, terrains, textured):
    """The wall 300 times with 300 sets of vertex colours: 376500 hits, every voxel a run of 300 equal keys (longer than a block of the merge
    kernel, and 1255 runs of 300 over 184 tiles cross blocks and tiles everywhere).  With a texture a third of whose texels are transparent, the
    runs have different lengths and sentinel keys are sorted behind them."""
    d, rules = work
    rng = np.random.default_rng(44)
    more, textures = {}, ()
    if textured:
        tex = rng.integers(0, 256, size=(16, 16, 4)).astype(np.uint8)
        tex[..., 3] = np.where(rng.random((16, 16)) < 1 / 3, 128, 255)
        more = {"uv": rng.uniform(0, 1, size=(3 * COPIES, 2)).astype(np.float32), "material": 0}
        textures = [tex]
    pos = np.tile(np.float32(WALL), (COPIES, 1))
    mesh = host.Mesh.from_arrays({"position": pos, "rgba": _rgba(rng, 3 * COPIES), **more}, textures=textures)
    c = stampmodel.counts(rules, mesh, WIDE, d)
    assert (c["pairs"] == 138).all() and (c["hits"] == 1255).all() and (c["kept"] == 1255).all()
    n = int(c["kept"].sum())
    assert n == 376500 > int(c["pairs"].sum()) and n > 100 * RADIX_TILE
    want, (x, y, z, _) = _model(work, terrains[WIDE], mesh, FILL)
    runs = np.unique(_keys(WIDE, x, y, z), return_counts=True)[1]
    if textured:
        assert len(x) == int(c["opaque"].sum()) and 0.5 * n < len(x) < 0.8 * n, "about a third of the hits are transparent"
        assert WAVE < runs.min() < runs.max(), "runs of different lengths"
    else:
        assert len(x) == n and len(runs) == 1255 and runs.min() == runs.max() == COPIES >= BLOCK + 1
    ctx = _uploaded(terrains[WIDE][2])
    try:
        assert ctx.stamp_mesh(mesh, FILL, 5) > 0.0
        _assert_levels(ctx, want, f"300 walls, textured {textured}")
    finally:
        ctx.close()
        want.close()


# ---- 5. the early exits ----------------------------------------------------------------------------------------------------------------------------

def test_stamps_that_leave_early_change_nothing(work, terrains):
    """Three stamps that end before the column pipeline: no triangle with area (no pairs), nothing kept (pairs, no hit) and every hit
    transparent (kept hits, no voxel).  All three return before the event that ends the measurement is recorded: 0.0 ms."""
    d, rules = work
    solid, colour, ws = terrains[WIDE]
    first = _mesh([FLAT], [[200, 100, 50, 255]] * 3)
    x, y, z, argb = stampmodel.voxelise(rules, first, WIDE, d)
    volume = stampmodel.apply_stamp(solid.copy(), colour.copy(), x, y, z, argb, FILL)
    edited = _world(*volume)
    no_area = _mesh([[[5, 5, 5], [5, 5, 5], [9, 20, 30]], [[3, 4, 5], [4, 6, 8], [5, 8, 11]], [[7, 7, 7], [7, 7, 7], [7, 7, 7]], [[60, 1, 2], [50, 1, 2], [40, 1, 2]]])
    outside = _mesh([[[300, 10, 300], [340, 10, 300], [300, 10, 340]], [[-50, 90, 20], [-40, 95, 30], [-45, 99, 25]]])
    tex = np.full((4, 4, 4), 200, dtype=np.uint8)
    quad = np.float32([[30, 20, 30], [60, 20, 30], [60, 25, 60], [30, 25, 60]])
    transparent = host.Mesh.from_arrays({"position": quad, "uv": np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]), "material": 0}, [0, 1, 2, 0, 2, 3], [tex])
    c = stampmodel.counts(rules, no_area, WIDE, d)
    assert (c["pairs"] == 0).all()
    c = stampmodel.counts(rules, outside, WIDE, d)
    assert (c["pairs"] > 0).all() and (c["hits"] == 0).all()
    c = stampmodel.counts(rules, transparent, WIDE, d)
    assert (c["kept"] > 100).all() and (c["opaque"] == 0).all()
    follow = _mesh([WALL], [[250, 10, 10, 255], [10, 250, 10, 255], [10, 10, 250, 255]])
    x, y, z, argb = stampmodel.voxelise(rules, follow, WIDE, d)
    after = _world(*stampmodel.apply_stamp(volume[0].copy(), volume[1].copy(), x, y, z, argb, FILL))
    ctx = _uploaded(ws)
    try:
        assert ctx.stamp_mesh(first, FILL, 5) > 0.0
        _assert_levels(ctx, edited, "the first stamp")
        before, stats = _levels(ctx), ctx.edit_stats()
        for label, mesh in (("no area", no_area), ("outside", outside), ("transparent", transparent)):
            for op in (FILL, CARVE, PAINT):
                assert ctx.stamp_mesh(mesh, op, 5) == 0.0, label
            assert _levels(ctx) == before, f"{label}: the world changed"
            assert ctx.edit_stats() == stats, label
        assert ctx.stamp_mesh(follow, FILL, 5) > 0.0
        _assert_levels(ctx, after, "the stamp after the early exits")
    finally:
        ctx.close()
        edited.close()
        after.close()


# ---- 6. triangles without columns around real ones -------------------------------------------------------------------------------------------------

def _gapped_mesh(work, total, gaps, ends):
    """`total` triangles: a real one, then for every gap that many triangles without area, one beyond the world's edge (clamped to it: box
    columns, no hit) and a real one; triangles without area up to the last, which is real.  ends: two triangles without area before and behind
    all that.  Returns the mesh and the kinds ('R'eal, 'D'egenerate, 'C'lamped)."""
    d, rules = work
    kinds = ["R"]
    for g in gaps:
        kinds += ["D"] * g + ["C", "R"]
    inner = total - (4 if ends else 0)
    if len(kinds) < inner:
        kinds += ["D"] * (inner - len(kinds) - 1) + ["R"]
    assert len(kinds) == inner and kinds[-1] == "R"
    if ends:
        kinds = ["D", "D"] + kinds + ["D", "D"]
    rng = np.random.default_rng(total)
    triangles = []
    for k, kind in enumerate(kinds):
        if kind == "R":
            centre = rng.uniform([8, 4, 8], [120, 56, 120])
            triangles.append(centre + rng.normal(0.0, 4.0, size=(3, 3)))
        elif kind == "C":
            triangles.append(np.array([[140, 10, 50], [150, 12, 52], [141, 11, 60]]) + [0, k % 40, k % 60])
        elif k % 2:
            a = rng.integers(0, 100, size=3)
            triangles.append([a, a, a + [3, 1, 2]])                   # a repeated corner
        else:
            a = rng.integers(0, 100, size=3)
            triangles.append([a, a + [1, 2, 3], a + [2, 4, 6]])       # collinear corners (small integers: the cross product is exactly 0)
    mesh = _mesh(triangles, _rgba(rng, 3 * total))
    c = stampmodel.counts(rules, mesh, WIDE, d)
    kinds = np.array(kinds)
    assert len(c) == total
    assert (c["pairs"][kinds == "D"] == 0).all(), "the triangles without area have no columns"
    assert (c["pairs"][kinds == "C"] > 0).all() and (c["hits"][kinds == "C"] == 0).all(), "the clamped triangles have columns and no hit"
    assert (c["kept"][kinds == "R"] > 0).all()
    return mesh, "".join(kinds)


GAPPED = [(BLOCK - 1, [1, 100], False), (BLOCK, [1], False), (BLOCK + 1, [1], True), (SCAN_CHUNK + 1, [1, BLOCK, BLOCK + 1], False),
          (SCAN_CHUNK + 1, [BLOCK], True), (4200, [SCAN_CHUNK, 1], False), (8200, [SCAN_CHUNK, 1], True)]


@pytest.mark.parametrize("total,gaps,ends", GAPPED)
def test_triangles_without_columns_first_last_and_in_blocks(work, terrains, total, gaps, ends):
    """TriangleOf finds a pair's triangle as the last one whose first pair is not behind it, so triangles without columns must share their
    successor's first pair: runs of 1, 256, 257 (a block of setup_kernel and one more) and 4096 (a chunk of the scan of the triangles' columns)
    of them between real triangles, in meshes of 255, 256, 257, 4097, 4200 and 8200 triangles, with real triangles first and last or (ends)
    triangles without area there.  The 4096 in a row need a mesh of at least 4098."""
    mesh, kinds = _gapped_mesh(work, total, gaps, ends)
    for g in gaps:
        assert "R" + "D" * g + "C" in kinds
    assert kinds.startswith("DDR" if ends else "R") and kinds.endswith("RDD" if ends else "R") and kinds.count("R") >= 3
    want, _ = _model(work, terrains[WIDE], mesh, FILL)
    ctx = _uploaded(terrains[WIDE][2])
    try:
        assert ctx.stamp_mesh(mesh, FILL, 5) > 0.0
        _assert_levels(ctx, want, f"{total} triangles, gaps {gaps}")
    finally:
        ctx.close()
        want.close()


# ---- 7. the bounding box ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voxels", [[(0, 40, 0), (0, 3, 0), (127, 30, 127), (127, 50, 127)], [(127, 45, 0)]])
def test_the_box_of_voxels_in_the_worlds_corners(work, terrains, voxels):
    """levelCount 0, so the rectangle is the voxels' box itself: one-hit triangles in columns (0, 0) and (127, 127) only (the whole world: every
    other column is rewritten as it was), then a single hit in column (127, 0) (one column)."""
    d, rules = work
    _, _, ws = terrains[WIDE]
    rng = np.random.default_rng(7)
    mesh = _mesh([_one_hit(v, 0.2) for v in voxels], _rgba(rng, 3 * len(voxels)))
    c = stampmodel.counts(rules, mesh, WIDE, d)
    assert (c["hits"] == 1).all()
    want, (x, y, z, _) = _model(work, terrains[WIDE], mesh, FILL)
    assert sorted(zip(x.tolist(), y.tolist(), z.tolist())) == sorted(voxels)
    ctx = _uploaded(ws)
    try:
        assert ctx.stamp_mesh(mesh, FILL, 0) > 0.0
        _assert_levels(ctx, want, f"hits at {voxels}", level_count=0, above=ws)
        assert ctx.read_region(0, 1, 1, 126, 126) == ws.extract_region(0, 1, 1, 126, 126), "the middle of the world changed"
    finally:
        ctx.close()
        want.close()


# ---- 8. slivers on the device ------------------------------------------------------------------------------------------------------------------------

def _sliver_obj(path, seed):
    """The mesh of tests/test_world_stamp_cpu.py::test_random_triangles_equal_the_host_voxeliser."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([_random_triangles(rng, 60), _slivers(rng, 24)])
    colours = rng.uniform(-0.1, 1.1, size=(len(pos), 3))
    return stampmodel.write_obj(path, pos, colours, [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(pos) // 3)])


def _outside_obj(path):
    """The mesh of tests/test_world_stamp_cpu.py::test_triangles_partly_outside_the_world."""
    rng = np.random.default_rng(5)
    pos = _random_triangles(rng, 40, spread=1.0, size=0.5)
    pos[:3] = [[-1.0, -1.0, -1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, 1.0]]
    faces = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(pos) // 3)]
    return stampmodel.write_obj(path, pos, rng.uniform(0, 1, size=(len(pos), 3)), faces)


@pytest.mark.parametrize("name,max_dimension,flip", [("slivers 1", 64, (True, False, False)), ("slivers 2", 64, (True, False, False)),
                                                      ("outside", 48, (True, True, False))])
def test_slivers_and_clamped_triangles_equal_the_host_voxeliser(work, tmp_path, name, max_dimension, flip):
    """The needles, collinear corners and NaN-barycentric slivers through the DEVICE's float rule (its NaN compares, ToInt, fminf / fmaxf), and
    triangles that reach past the world: the stamped empty world is host.WorldSet.from_obj of the same file, the independent host voxeliser."""
    d, rules = work
    path = str(tmp_path / "mesh.obj")
    path = _outside_obj(path) if name == "outside" else _sliver_obj(path, int(name.split()[1]))
    mesh = host.Mesh.from_obj(path)
    dims = mesh.rescale(max_dimension, flip)
    want = host.WorldSet.from_obj(path, max_dimension, flip=flip)
    assert tuple(want.dims) == tuple(dims)
    c = stampmodel.counts(rules, mesh, dims, d)
    if name == "outside":
        assert len(c) == 40 and (mesh.vertices["position"].max(axis=0) > np.array(dims) - 1).any(), "some triangle reaches past the last voxel"
    else:
        assert len(c) == 84 and c["kept"][60:].sum() > 0, "at least one sliver has hits"
        assert (c["pairs"][60:] == 0).any(), "and some have no area at all"
    empty = _empty(dims)
    ctx = _uploaded(empty)
    try:
        assert ctx.stamp_mesh(mesh, FILL, 5) > 0.0
        _assert_levels(ctx, want, name)
    finally:
        ctx.close()
        want.close()
        empty.close()


# ---- 9. the format limit ---------------------------------------------------------------------------------------------------------------------------

def test_a_stamped_column_over_the_format_limits_is_rejected_whole(work):
    """A wall through all 32768 heights of one column of the world of tests/test_gpu_world_edit_rejections.py's over-limit test: FILL would
    make a run of 32768 voxels there, which the stamp's own count kernel flags (CVX_ERR_CAPACITY, nothing written); CARVE with the same mesh
    fits."""
    d, rules = work
    dims = (32, 32768, 32)
    xs, zs = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    xs, zs = xs.ravel(), zs.ravel()
    ys = (xs * 7 + zs * 3) % 50
    ws = host.WorldSet.from_voxels(dims, xs.astype(np.int32), ys.astype(np.int32), zs.astype(np.int32), _colour(xs, ys, zs), threads=4)
    mesh = _mesh([[[3.5, -1, 3.2], [3.5, 100000, 5.0], [3.5, -1, 6.9]]], [[250, 10, 10, 255], [10, 250, 10, 255], [10, 10, 250, 255]])
    c = stampmodel.counts(rules, mesh, dims, d)[0]
    assert (c["pairs"], c["hits"], c["kept"], c["column_max"]) == (10, 103256, 103256, 32768) and c["column_max"] == dims[1] > 32767
    x, y, z, argb = stampmodel.voxelise(rules, mesh, dims, d)
    solid = np.zeros(dims, dtype=bool)
    solid[xs, ys, zs] = True
    assert solid[x, y, z].any(), "CARVE has something to remove"
    after = _world(*stampmodel.apply_stamp(solid, _dense(solid), x, y, z, argb, CARVE))
    ctx = _uploaded(ws)
    try:
        before = ctx.read_level(0)[0]
        assert before == ws.storage(0).tobytes()
        stats = ctx.edit_stats()
        with pytest.raises(gpu.CvxError, match=r"error -4: a stamped column would need .* a run longer than 32767 voxels"):
            ctx.stamp_mesh(mesh, FILL, 5)
        assert ctx.read_level(0)[0] == before
        assert ctx.edit_stats() == stats
        assert ctx.stamp_mesh(mesh, CARVE, 5) > 0.0
        _assert_levels(ctx, after, "CARVE after the rejected FILL")
    finally:
        ctx.close()
        ws.close()
        after.close()
