"""GPU: where placed voxel models touch the device-resident world (cvxc_world_contacts[_device], include/cpuvox_gpu_contacts.h).

A call is made on a context and, independently, on the numpy model (tests/contactsmodel.py): results, points and summary must be equal byte for
byte.  Everything is integers: no comparison has a tolerance.  The worlds are the 128 x 64 x 128 terrain and the 32 x 256 x 32 tall world of
tests/test_gpu_world_dense.py (with one more run, across y = 192), a flat 32 x 32 x 32 world and the 32 x 64 x 256 world of tests/oblongworlds.py.
Every case asserts from the model that its input has the property it is named for before it calls the device."""
import numpy as np
import pytest
import torch

import contactsmodel
import oblongworlds
import pickmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _dense
from test_gpu_world_dense import TALL, _any_world, _tall_solid
from test_gpu_world_edit import DIMS, _terrain
from test_world_contacts_cpu import CUBE, colour_of, cube_model, flat_world, same
from test_world_models_cpu import as_dicts, forward_about_centre, identity_at, mixed_call, random_model, rotation, tilt

pytestmark = pytest.mark.gpu

DEFAULT = gpu.SURFACE_OUTSIDE_DEFAULT
FLAT = (32, 32, 32)
SENTINEL = 0xA5


class World:
    """A world on the host and in a context of its own; the calls under test never write it."""

    def __init__(self, dims, solid, colour):
        self.dims, self.solid, self.colour = dims, solid, colour
        self.ws = _any_world(dims, solid, colour)
        self.ctx = gpu.Context(0)
        self.ctx.upload_world(self.ws)

    def close(self):
        self.ctx.close()
        self.ws.close()

    def model(self, models, instances, solid_outside=DEFAULT):
        return contactsmodel.contacts(self.solid, self.colour, models, as_dicts(instances), solid_outside)


def _fixture(make):
    @pytest.fixture(scope="module")
    def world():
        w = World(*make())
        yield w
        w.close()
    return world


def _with_colour(dims, solid):
    return dims, solid, _dense(solid)


terrain = _fixture(lambda: _with_colour(DIMS, _terrain()))


def _tall_with_a_run_across_192():
    """tests/test_gpu_world_dense.py's tall world, whose highest run ends at 190, with one more run, [180, 200), in six columns."""
    solid = _tall_solid()
    solid[10:12, 180:200, 10:13] = True
    return solid


tall = _fixture(lambda: _with_colour(TALL, _tall_with_a_run_across_192()))
flat = _fixture(lambda: (FLAT, *flat_world(dims=FLAT)))
walled = _fixture(lambda: (FLAT, *flat_world(wall=True, dims=FLAT)))
oblong = _fixture(lambda: (oblongworlds.LONG_Z, *oblongworlds.volumes(oblongworlds.LONG_Z)))


def _device_models(models):
    """Host models as world_contacts_device takes them, and the tensors that hold their arrays."""
    keep, out = [], []
    for argb, mask in models:
        shape = (argb if argb is not None else mask).shape
        a = torch.from_numpy(np.ascontiguousarray(argb, dtype=np.uint32).view(np.int32)).cuda() if argb is not None else None
        m = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).cuda() if mask is not None else None
        keep += [a, m]
        out.append(((shape[0], shape[2], shape[1]), a.data_ptr() if a is not None else 0, m.data_ptr() if m is not None else 0))
    torch.cuda.synchronize()
    return out, keep


def _device_call(ctx, models, instances, solid_outside, capacity, spare=0):
    """One device call into sentinel-filled tensors -> (results, the points tensor's entries as an array, totals)."""
    descriptors, keep = _device_models(models)
    results = torch.full((len(instances) * 120,), SENTINEL, dtype=torch.uint8, device="cuda")
    points = torch.full(((capacity + spare) * 24,), SENTINEL, dtype=torch.uint8, device="cuda") if capacity + spare else None
    torch.cuda.synchronize()
    if points is not None and spare:  # (the wrapper takes the tensor's size for the capacity: hand it the first `capacity` entries)
        totals, ms = ctx.world_contacts_device(descriptors, instances, results, points[:capacity * 24] if capacity else None, solid_outside)
    else:
        totals, ms = ctx.world_contacts_device(descriptors, instances, results, points, solid_outside)
    assert ms > 0.0
    listed = points.cpu().numpy().view(gpu.CONTACT_POINT_DTYPE) if points is not None else np.zeros(0, dtype=gpu.CONTACT_POINT_DTYPE)
    return results.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE), listed, totals


def _check(world, models, instances, solid_outside=DEFAULT, what="", device=True):
    """The host call, and the device call, against the model; returns the model's answer."""
    want = world.model(models, instances, solid_outside)
    results, points, totals, ms = world.ctx.world_contacts(models, instances, solid_outside)
    assert ms > 0.0
    same((results, points, totals), want, what)
    if device:
        same(_device_call(world.ctx, models, instances, solid_outside, want[2]["points"]), want, what + " (device)")
    return want


# ---- 1. the mixed call ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("world_name", ["terrain", "tall"])
def test_the_mixed_call_equals_the_model(terrain, tall, world_name):
    world = terrain if world_name == "terrain" else tall
    names, models, instances = mixed_call(np.random.default_rng(11), world.dims, gpu.BRUSH_FILL)
    want = world.model(models, instances)
    results = want[0]
    assert (results["overlap"] > 0).any() and (results["normal"] != 0).any(axis=1).any() and want[2]["points"] > 0
    d = as_dicts(instances)[names["partly outside"]]
    assert any(d["box_min"][a] < 0 or d["box_max"][a] > world.dims[a] for a in range(3))
    assert instances[names["tall"]].boxMax[1] - instances[names["tall"]].boxMin[1] > 64, "more than one step"
    _check(world, models, instances, what=world_name)


# ---- 2. hand-made cases on flat ground --------------------------------------------------------------------------------------------------------------

def test_flat_ground_cases(flat):
    models = [cube_model()]
    cube = lambda at: identity_at(at, CUBE, 0, gpu.BRUSH_FILL)  # noqa: E731
    names = ["bottom layer", "two layers", "in air", "buried", "below the world"]
    instances = [cube((6, 7, 6)), cube((12, 6, 20)), cube((20, 12, 6)), cube((6, 2, 20)), cube((20, -2, 20))]
    for so in (DEFAULT, 0):
        results, points, summary = _check(flat, models, instances, so, f"solidOutside {so}")
        r = dict(zip(names, results))
        assert (r["bottom layer"]["voxels"], r["bottom layer"]["overlap"], r["bottom layer"]["points"]) == (64, 16, 16) and r["bottom layer"]["normal"].tolist() == [0, 16, 0]
        assert (points["faces"][points["instance"] == 0] == 0x08).all() and gpu.contact_response(r["bottom layer"])[2] == 1.0
        assert (r["two layers"]["overlap"], r["two layers"]["points"]) == (32, 16) and gpu.contact_response(r["two layers"])[2] == 2.0
        assert r["in air"]["overlap"] == 0 and not r["in air"]["max"].any() and r["in air"]["voxels"] == 64
        assert (r["buried"]["overlap"], r["buried"]["points"]) == (64, 0) and not r["buried"]["normal"].any()
        if so == DEFAULT:
            assert (r["below the world"]["overlap"], r["below the world"]["points"]) == (64, 0)
        else:
            assert (r["below the world"]["overlap"], r["below the world"]["points"]) == (32, 16) and r["below the world"]["normal"].tolist() == [0, -16, 0]
        assert summary["touching"] == 4


def test_a_wall_corner_gives_a_two_axis_normal(walled):
    """The cube one layer in a wall (x < 6, up to y = 20) and one layer in the ground at once: the wall's voxels have +X open, the ground's +Y."""
    corner = identity_at((5, 7, 8), CUBE, 0, gpu.BRUSH_FILL)
    results, points, summary = _check(walled, [cube_model()], [corner], 0x04, "the wall corner")
    assert results["overlap"][0] == 16 + 12 and results["normal"][0].tolist() == [12, 12, 0] and set(points["faces"].tolist()) == {0x02, 0x08}
    assert (points["voxel"][points["faces"] == 0x02][:, 0] == 5).all() and (points["voxel"][points["faces"] == 0x08][:, 1] == 7).all()
    assert summary == dict(touching=1, overlap=28, points=24, voxels=64)


# ---- 3. against the existing calls alone ------------------------------------------------------------------------------------------------------------

def test_against_read_place_and_surface_alone():
    """No model: B_k is where a FILL of the instance wrote its marker colour, O_k those of them that were solid before; the faces of every point
    are the faces cvx_world_surface lists for that voxel."""
    solid = _terrain()
    colour = _dense(solid)
    marker = 0xFFABCDEF
    assert not (colour == marker).any()
    size = (9, 11, 7)
    mask = random_model(np.random.default_rng(2), size, with_mask=True, zeros=0.3)[1]
    model = (np.full(mask.shape, marker, dtype=np.uint32), mask)
    cx, cz = 40, 70
    surface = int(np.nonzero(solid[cx, :, cz])[0].max())
    inst = gpu.model_instance(forward_about_centre(rotation(1, 35) @ rotation(0, 20), size, (cx, surface, cz)), size, 0, gpu.BRUSH_FILL)
    lo, hi = list(inst.boxMin), list(inst.boxMax)
    assert all(lo[a] > 0 and hi[a] < DIMS[a] for a in range(3)), "inside the world"
    world = World(DIMS, solid, colour)
    try:
        ctx = world.ctx
        results, points, totals, _ = ctx.world_contacts([model], [inst], DEFAULT)
        quads, _, _ = ctx.world_surface(lo, hi, DEFAULT, gpu.SURFACE_IGNORE_COLOUR)
        before_argb, before_solid = ctx.read_voxels(lo, hi)
        ctx.place_models([model], [inst], 0)
        after_argb, _ = ctx.read_voxels(lo, hi)
    finally:
        world.close()
    body = after_argb == marker  # (X, Z, Y)
    overlap = body & before_solid
    r = results[0]
    assert 0 < overlap.sum() < body.sum() and (r["voxels"], r["overlap"]) == (body.sum(), overlap.sum())
    x, z, y = np.nonzero(overlap)
    assert r["sum"].tolist() == [x.sum(), y.sum(), z.sum()] and r["origin"].tolist() == lo
    assert r["min"].tolist() == [lo[0] + x.min(), lo[1] + y.min(), lo[2] + z.min()] and r["max"].tolist() == [lo[0] + x.max() + 1, lo[1] + y.max() + 1, lo[2] + z.max() + 1]
    faces = np.zeros(body.shape, dtype=np.int32)
    for q in quads:
        qx, qy, qz = (int(q["voxel"][a]) - lo[a] for a in range(3))
        faces[qx, qz, qy:qy + int(q["length"])] |= 1 << int(q["face"])
    listed = overlap & (faces != 0)
    assert totals["points"] == len(points) == listed.sum() > 0
    px, py, pz = (points["voxel"][:, a] - lo[a] for a in range(3))
    assert overlap[px, pz, py].all() and (points["faces"] == faces[px, pz, py]).all() and (points["argb"] == before_argb[px, pz, py]).all()
    assert r["normal"].tolist() == [int(((faces >> (2 * a + 1) & 1) * overlap).sum()) - int(((faces >> (2 * a) & 1) * overlap).sum()) for a in range(3)]


# ---- 4. the seams of the steps ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("solid_outside", [0x04, 0x08, 0])
def test_step_seams(tall, solid_outside):
    """Boxes over y in [-3, 259) (steps that end at 2 | 3, 66 | 67, 130 | 131, 194 | 195) and [0, 256) (63 | 64, 127 | 128, 191 | 192) with a model
    whose every voxel is set, over columns of the tall world whose runs end at 63 | 64 and 127 | 128 and cross 192."""
    at, footprint = (8, 9), (6, 6)
    columns = tall.solid[at[0]:at[0] + footprint[0], :, at[1]:at[1] + footprint[1]]
    ends = lambda y: (columns[:, y - 1, :] != columns[:, y, :]).any()  # noqa: E731
    assert ends(64) and ends(128) and (columns[:, 191, :] & columns[:, 192, :]).any() and not ends(192)
    for y in (2, 3, 66, 67, 130, 131, 194, 195, 63, 64, 127, 128, 191, 192):
        assert columns[:, y, :].any(), f"solid voxels on both sides of every seam (y = {y})"
    instances, models = [], []
    for k, (y0, y1) in enumerate(((-3, 259), (0, 256))):
        size = (footprint[0], y1 - y0, footprint[1])
        models.append((None, np.ones((size[0], size[2], size[1]), dtype=bool)))
        instances.append(identity_at((at[0], y0, at[1]), size, k, gpu.BRUSH_FILL))
    results, points, _ = _check(tall, models, instances, solid_outside, f"solidOutside {solid_outside}")
    assert results["voxels"].tolist() == [36 * 262, 36 * 256]
    assert (results["overlap"][0] - results["overlap"][1]) == 36 * (3 * bool(solid_outside & 0x04) + 3 * bool(solid_outside & 0x08))
    for y in (66, 67, 130, 131, 194, 195, 63, 64, 127, 128, 191, 192):  # (y = 2 and 3 lie inside the ground: overlap without an open face)
        assert (points["voxel"][:, 1] == y).any(), f"points on both sides of every seam (y = {y})"


def test_boxes_far_taller_than_their_bodies(terrain):
    """Boxes stretched to 3000 voxels of height: a wave cuts its steps to the part of its column's line that can meet the model, and the answer
    is that of the helper's box, but for origin and the sums relative to it."""
    size = (9, 11, 7)
    model = random_model(np.random.default_rng(8), size, zeros=0.3)
    snug, tall_ones = [], []
    for linear, (cx, cz) in ((tilt(), (40, 40)), (rotation(0, 90), (64, 90)), (rotation(1, 90), (90, 30)), (2 * rotation(1, 30), (20, 100)), (np.diag([1.0, -1.0, 1.0]), (100, 100))):
        surface = int(np.nonzero(terrain.solid[cx, :, cz])[0].max())
        snug.append(gpu.model_instance(forward_about_centre(linear, size, (cx, surface, cz)), size, 0, gpu.BRUSH_FILL))
        stretched = gpu.model_instance(forward_about_centre(linear, size, (cx, surface, cz)), size, 0, gpu.BRUSH_FILL)
        stretched.boxMin[1] -= 1000
        stretched.boxMax[1] += 2000
        tall_ones.append(stretched)
    want = _check(terrain, [model], snug + tall_ones, DEFAULT, "stretched boxes")[0]
    assert (want["overlap"][:5] > 0).all() and (want["normal"][:5] != 0).any(axis=1).all()
    for name in ("voxels", "overlap", "points", "normal", "min", "max"):
        assert (want[name][:5] == want[name][5:]).all(), name
    assert (want["sum"][5:, 1] == want["sum"][:5, 1] + 1000 * want["overlap"][:5].astype(np.uint64)).all()


# ---- 5. the world's edges ---------------------------------------------------------------------------------------------------------------------------

def test_world_edges(terrain):
    dims, solid = terrain.dims, terrain.solid
    models = [cube_model()]
    at_x = identity_at((-2, int(np.nonzero(solid[0, :, 60])[0].max()) - 1, 60), CUBE, 0, gpu.BRUSH_FILL)
    at_z = identity_at((60, int(np.nonzero(solid[60, :, dims[2] - 1])[0].max()) - 1, dims[2] - 2), CUBE, 0, gpu.BRUSH_FILL)
    assert at_x.boxMin[0] < 0 < at_x.boxMax[0] and at_z.boxMin[2] <= dims[2] - 1 < at_z.boxMax[2] - 1
    answers = {so: _check(terrain, models, [at_x, at_z], so, f"solidOutside {so:#x}")[0] for so in (0, 0x01, 0x20, 0x21)}
    assert answers[0]["overlap"].min() > 0
    for k, bit, axis in ((0, 0x01, 0), (1, 0x20, 2)):
        without, with_bit = answers[0][k], answers[bit][k]
        assert with_bit["overlap"] > without["overlap"], "the voxels beyond the edge are solid with the bit"
        assert without["normal"][axis] != with_bit["normal"][axis], "the faces across the edge change"
        other = answers[0x21 ^ bit][k].copy()  # (the other instance's bit alone: nothing but the place in the list may change)
        other["firstPoint"] = without["firstPoint"]
        assert other.tobytes() == without.tobytes(), "the other face's bit changes nothing here"
    assert answers[0x21][0]["overlap"] == answers[0x01][0]["overlap"] and answers[0x21][1]["overlap"] == answers[0x20][1]["overlap"]


# ---- 6. capacities ----------------------------------------------------------------------------------------------------------------------------------

def test_capacities(terrain):
    names, models, instances = mixed_call(np.random.default_rng(11), terrain.dims, gpu.BRUSH_FILL)
    want = terrain.model(models, instances)
    total = want[2]["points"]
    assert total > 10
    spare = 7
    for capacity in (0, total - 1, total, total + 5):
        results, listed, totals = _device_call(terrain.ctx, models, instances, DEFAULT, capacity, spare)
        assert results.tobytes() == want[0].tobytes() and totals == want[2], f"capacity {capacity}: results and summary"
        n = min(capacity, total)
        assert listed[:n].tobytes() == want[1][:n].tobytes(), f"capacity {capacity}: the listed prefix"
        assert (listed[n:].view(np.uint8) == SENTINEL).all() and len(listed) == capacity + spare, f"capacity {capacity}: entries beyond are left alone"
        host_results, host_points, host_totals, _ = terrain.ctx.world_contacts(models, instances, DEFAULT, capacity)
        assert host_results.tobytes() == want[0].tobytes() and host_totals == want[2] and host_points.tobytes() == want[1][:n].tobytes()


# ---- 7. the pair lookup and the atomics -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 64, 65, 4096])
def test_pair_lookup_and_atomics(terrain, count):
    """`count` instances with one-column boxes around one 48 x 48-footprint instance (2304 waves on one result) that is there twice."""
    dims, solid = terrain.dims, terrain.solid
    rng = np.random.default_rng(count)
    slab = (48, 6, 48)
    models = [(None, np.ones((1, 1, 8), dtype=bool)), random_model(rng, slab, zeros=0.2)]
    big = identity_at((30, int(np.nonzero(solid[54, :, 54])[0].max()) - 2, 30), slab, 1, gpu.BRUSH_FILL)
    assert (big.boxMax[0] - big.boxMin[0]) * (big.boxMax[2] - big.boxMin[2]) == 2304
    instances = []
    for k in range(count - 2 if count > 2 else count):
        x, z = int(rng.integers(0, dims[0])), int(rng.integers(0, dims[2]))
        instances.append(identity_at((x, int(np.nonzero(solid[x, :, z])[0].max()) - int(rng.integers(0, 8)), z), (1, 8, 1), 0, gpu.BRUSH_FILL))
    if count > 2:
        instances.insert(count // 3, big)
        instances.insert(2 * count // 3, big)
    assert len(instances) == count
    want = _check(terrain, models, instances, DEFAULT, f"{count} instances", device=count <= 65)
    assert (want[0]["overlap"] > 0).sum() > count // 2
    if count > 2:
        a, b = want[0][count // 3].copy(), want[0][2 * count // 3 + 0].copy()
        assert a["overlap"] > 100 and a["firstPoint"] != b["firstPoint"]
        a["firstPoint"] = b["firstPoint"] = 0
        assert a.tobytes() == b.tobytes(), "two identical instances give identical results"
    first = terrain.ctx.world_contacts(models, instances, DEFAULT)
    again = terrain.ctx.world_contacts(models, instances, DEFAULT)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2], "the same call twice gives the same bytes"


def test_more_pairs_than_the_launch_has_waves(terrain):
    """A 520 x 520 footprint, 270 400 pairs: beyond 2^18 the waves of the launch take the pairs in turn."""
    slab = (520, 3, 520)
    models = [random_model(np.random.default_rng(6), slab, zeros=0.5), (None, np.ones((1, 1, 8), dtype=bool))]
    surface = int(np.nonzero(terrain.solid[64, :, 64])[0].max())
    wide = identity_at((-196, surface - 1, -196), slab, 0, gpu.BRUSH_FILL)
    last = identity_at((64, surface - 3, 64), (1, 8, 1), 1, gpu.BRUSH_FILL)
    assert (wide.boxMax[0] - wide.boxMin[0]) * (wide.boxMax[2] - wide.boxMin[2]) > 1 << 18
    want = _check(terrain, models, [wide, last], 0x04 | 0x20, "270 400 pairs")
    assert want[0]["overlap"][0] > 100000 and want[0]["max"][0][2] > terrain.dims[2] and want[0]["overlap"][1] > 0 and want[2]["points"] > 1000


# ---- 8. the loop: carve, lift, test where the body rests --------------------------------------------------------------------------------------------

def test_a_lifted_piece_rests_where_the_model_says():
    dims = (32, 64, 32)
    solid = np.zeros(dims, dtype=bool)
    solid[:, :8, :] = True
    solid[10:18, 8:30, 12:20] = True  # a pillar on the ground ...
    solid[8:20, 30:36, 10:22] = True  # ... with a wider head
    colour = colour_of(solid)
    neck = [{"op": gpu.BRUSH_CARVE, "shape": 0, "a": (0, 24, 0), "b": (32, 28, 32), "argb": 0}]
    world = World(dims, solid.copy(), colour.copy())
    try:
        ctx = world.ctx
        ctx.brush(neck, 5)
        pickmodel.apply_strokes(world.solid, world.colour, neck)
        argb = torch.zeros(4096, dtype=torch.int32, device="cuda")
        mask = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pieces, summary, _ = ctx.world_lift_pieces_device((0, 0, 0), dims, gpu.ANCHOR_GROUND, argb, mask, gpu.LIFT_REMOVE, 5, 16, 4096)
        assert len(pieces) == 1 and summary["storedPieces"] == 1 and pieces[0]["piece"]["min"].tolist() == [8, 28, 10]
        lifted = gpu.lifted_model(pieces, 0, argb.data_ptr(), mask.data_ptr())
        size = lifted[0]
        assert size == (12, 8, 12)
        n = size[0] * size[1] * size[2]
        host_model = (argb.cpu().numpy().view(np.uint32)[:n].reshape(size[0], size[2], size[1]), mask.cpu().numpy()[:n].reshape(size[0], size[2], size[1]).astype(bool))
        world.solid[8:20, 28:36, 10:22] &= ~host_model[1].transpose(0, 2, 1)  # the REMOVE
        world.colour[~world.solid] = 0
        assert not world.solid[:, 28:, :].any() and world.solid[10:18, 23, 12:20].all() and not world.solid[10:18, 24, 12:20].any()
        at = lambda y: identity_at((8, y, 10), size, 0, gpu.BRUSH_FILL)  # noqa: E731
        instances = [at(28), at(25), at(23), at(22)]  # where it was, in the air, resting one layer into the pillar's stump, two layers
        want = world.model([host_model], instances)
        assert want[0]["overlap"].tolist()[:2] == [0, 0] and want[0]["overlap"][2] == 64 and want[0]["overlap"][3] == 128
        assert want[0]["normal"][2].tolist() == [0, 64, 0] and gpu.contact_response(want[0][3])[2] == 2.0
        results = torch.zeros(len(instances) * 120, dtype=torch.uint8, device="cuda")
        points = torch.zeros(want[2]["points"] * 24, dtype=torch.uint8, device="cuda")
        totals, ms = ctx.world_contacts_device([lifted], instances, results, points)
        same((results.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE), points.cpu().numpy().view(gpu.CONTACT_POINT_DTYPE), totals), want, "the lifted piece")
    finally:
        world.close()


# ---- 9. ordering and purity -------------------------------------------------------------------------------------------------------------------------

def test_the_call_sees_a_stroke_before_it_and_writes_nothing():
    solid, colour = flat_world(dims=FLAT)
    world = World(FLAT, solid.copy(), colour.copy())
    try:
        models = [cube_model()]
        instances = [identity_at((10, 8, 10), CUBE, 0, gpu.BRUSH_FILL)]
        before = world.model(models, instances)
        stroke = [{"op": gpu.BRUSH_FILL, "shape": 0, "a": (8, 8, 8), "b": (12, 10, 16), "argb": 0xFF102030}]
        pickmodel.apply_strokes(world.solid, world.colour, stroke)
        after = world.model(models, instances)
        assert before[0]["overlap"][0] == 0 and after[0]["overlap"][0] == 2 * 2 * 4 and after[0]["normal"][0].tolist() == [8, 8, 0]
        world.ctx.brush(stroke, 5)
        results, points, totals, _ = world.ctx.world_contacts(models, instances)
        same((results, points, totals), after, "behind the stroke")
        assert (points["argb"] == 0xFF102030).all()
        levels = [world.ctx.read_level(k) for k in range(6)]
        stats = world.ctx.edit_stats()
        world.ctx.world_contacts(models, instances)
        _device_call(world.ctx, models, instances, DEFAULT, totals["points"])
        assert [world.ctx.read_level(k) for k in range(6)] == levels and world.ctx.edit_stats() == stats, "every level reads as before"
    finally:
        world.close()


# ---- 10. an oblong world, and one that repeats ------------------------------------------------------------------------------------------------------

def test_oblong_and_repeating_worlds(oblong):
    dims = oblong.dims
    assert dims[0] != dims[2]
    names, models, instances = mixed_call(np.random.default_rng(13), dims, gpu.BRUSH_FILL)
    far = gpu.model_instance(forward_about_centre(tilt(), (9, 11, 7), (dims[0] - 3, 14, dims[2] - 4)), (9, 11, 7), 0, gpu.BRUSH_FILL)  # beyond both far faces
    wrapped = gpu.model_instance(forward_about_centre(rotation(1, 45), (9, 11, 7), (dims[0] + 16, 10, dims[2] // 2)), (9, 11, 7), 0, gpu.BRUSH_FILL)  # wholly beyond +X
    instances += [far, wrapped]
    for so in (DEFAULT, 0x04 | 0x02):
        want = _check(oblong, models, instances, so, f"oblong, solidOutside {so:#x}")
        assert (want[0]["overlap"] > 0).sum() >= 3 and want[0]["max"][-2][2] > 32, "overlap at z beyond the short side's length"
        assert wrapped.boxMin[0] >= dims[0] and (want[0]["overlap"][-1] > 0) == bool(so & 0x02), "beyond +X the outside rule decides, not the wrapped world"
    # inside the world at the same place modulo dimX the model would touch the terrain
    moved = gpu.model_instance(forward_about_centre(rotation(1, 45), (9, 11, 7), (16, 10, dims[2] // 2)), (9, 11, 7), 0, gpu.BRUSH_FILL)
    assert oblong.model(models, [moved])[0]["overlap"][0] > 0
    oblong.ctx.set_world_repeat(True)
    try:
        want = oblong.model(models, instances)
        results, points, totals, _ = oblong.ctx.world_contacts(models, instances)
        same((results, points, totals), want, "a repeating world does not wrap coordinates")
        assert results["overlap"][-1] == 0
    finally:
        oblong.ctx.set_world_repeat(False)


# ---- 11. errors -------------------------------------------------------------------------------------------------------------------------------------

def test_errors_leave_the_world_and_the_next_call_alone(flat):
    models = [cube_model()]
    good = identity_at((6, 7, 6), CUBE, 0, gpu.BRUSH_FILL)
    want = flat.model(models, [good])
    levels = [flat.ctx.read_level(k) for k in range(6)]

    def changed(**fields):
        inst = identity_at((6, 7, 6), CUBE, 0, gpu.BRUSH_FILL)
        for name, (index, value) in fields.items():
            getattr(inst, name)[index] = value
        return inst
    bad_model = identity_at((6, 7, 6), CUBE, 1, gpu.BRUSH_FILL)
    big_m = identity_at((6, 7, 6), CUBE, 0, gpu.BRUSH_FILL)
    big_m.toModel.m[0][0] = (1 << 24) + 1
    far_t = identity_at((6, 7, 6), CUBE, 0, gpu.BRUSH_FILL)
    far_t.toModel.t[2] = (1 << 46) + 1
    wide = changed(boxMin=(0, -(1 << 16)), boxMax=(0, 1 << 16))
    wide.boxMin[2], wide.boxMax[2] = -(1 << 16), 1 << 16
    for instances, so, capacity, message in (
            ([bad_model], DEFAULT, None, "instance 0: model 1 outside 0 .. 0"), ([changed(boxMax=(1, 7))], DEFAULT, None, r"instance 0: the box \[7, 7\) on axis 1 is empty"),
            ([good, changed(boxMin=(2, -(1 << 30) - 1))], DEFAULT, None, "instance 1: the box .* beyond 2\\^30"), ([big_m], DEFAULT, None, "toModel: m\\[0\\]\\[0\\]"),
            ([good], 0x40, None, "unknown solidOutside bits 0x40"), ([good], DEFAULT, -1, "pointCapacity -1"), ([], DEFAULT, None, "instanceCount 0"),
            ([good] * 4097, DEFAULT, None, "instanceCount 4097"), ([wide], DEFAULT, None, "error -4.*footprints sum to"),
            ([identity_at((6, 7, 6), CUBE, -1, gpu.BRUSH_FILL)], DEFAULT, None, "instance 0: model -1 outside 0 .. 0"), ([far_t], DEFAULT, None, "toModel: t\\[2\\]")):
        with pytest.raises(gpu.CvxError, match=message):
            flat.ctx.world_contacts(models, instances, so, capacity)
    for bad_models, message in (([], "modelCount 0 outside"), (models * 257, "modelCount 257 outside")):
        with pytest.raises(gpu.CvxError, match=message):
            flat.ctx.world_contacts(bad_models, [good])
    results_tensor = torch.zeros(120, dtype=torch.uint8, device="cuda")
    for size, message in (((2, 0, 2), "model 0: size 0 on axis 1 is below 1"), ((2048, 2048, 512), "model 0: 2\\^31 or more voxels")):
        with pytest.raises(gpu.CvxError, match=message):
            flat.ctx.world_contacts_device([(size, results_tensor.data_ptr(), 0)], [good], results_tensor)
    with pytest.raises(gpu.CvxError, match="models NULL or modelCount 1"):
        flat.ctx._contacts(lambda h, descriptors, *rest: gpu.lib().cvxc_world_contacts(h, None, *rest), gpu.Context._models(models, "test")[0], 1, [good], DEFAULT, 1, None, 0)
    with pytest.raises(gpu.CvxError, match="model 0: argb and solid are both NULL"):
        flat.ctx.world_contacts_device([(CUBE, 0, 0)], [good], torch.zeros(120, dtype=torch.uint8, device="cuda"))
    with pytest.raises(gpu.CvxError, match="results is NULL"):
        flat.ctx._contacts(gpu.lib().cvxc_world_contacts, gpu.Context._models(models, "test")[0], 1, [good], DEFAULT, None, None, 0)
    with pytest.raises(gpu.CvxError, match="pointCapacity 3 with no list"):
        flat.ctx._contacts(gpu.lib().cvxc_world_contacts_device, gpu.Context._models(models, "test")[0], 1, [good], DEFAULT, 1, None, 3)
    results, points, totals, _ = flat.ctx.world_contacts(models, [good])
    same((results, points, totals), want, "after the rejected calls")
    assert [flat.ctx.read_level(k) for k in range(6)] == levels
    empty = gpu.Context(0)
    try:
        with pytest.raises(gpu.CvxError, match="error -3.*not been uploaded"):
            empty.world_contacts(models, [good])
    finally:
        empty.close()
