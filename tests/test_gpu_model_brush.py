"""GPU: cvxd_models_brush / cvxd_models_brush_device (include/cpuvox_gpu_model_brush.h).  Every case of tests/modelbrushcases.py -- the ones
tests/test_model_brush_cpu.py runs through the host rules -- goes through the host call and through the device call on torch tensors, and both
are compared byte for byte with the numpy model of tests/modelbrushmodel.py, the sequential definition: the models' arrays, the model results,
the instance results and the summary; each case first asserts from the model the property it is named for.  Then the call is composed with the
calls that exist: cvxp_model_contacts' overlap with a rasterised stroke is the instance's `carved` before the call and 0 after it, under every
map; on a lifted piece the sums are cvx_world_lift_pieces' and cvxd_model_mass is cvx_lifted_piece_mass moved by piece.min; after a PAINT
cvxv_models_draw shows the new colour where cvxq_model_pick names a painted voxel.  Everything is integers: no tolerance."""
import numpy as np
import pytest
import torch

import modelbrushcases
import modelbrushmodel
import scenes
from cpuvox_amd import gpu
from modelbrushcases import BLUE, CARVE, PAINT, RED, box, sphere
from test_model_brush_cpu import same
from test_world_models_cpu import as_dicts, identity_at

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    """A fresh context: no world is ever uploaded into it."""
    context = gpu.Context(0)
    yield context
    context.close()


def _tensors(models):
    """Host models as models_brush_device takes them: (argb, solid) tensors on the device."""
    out = []
    for argb, mask in models:
        a = torch.from_numpy(np.ascontiguousarray(argb, dtype=np.uint32).view(np.int32).copy()).cuda() if argb is not None else None
        m = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).cuda() if mask is not None else None
        out.append((a, m))
    torch.cuda.synchronize()
    return out


def _back(tensors):
    return [(a.cpu().numpy().view(np.uint32) if a is not None else None, (m.cpu().numpy() != 0) if m is not None else None) for a, m in tensors]


def _both(ctx, models, instances, strokes, want, what):
    """The host call and the device call against `want`, the model's answer; the caller's arrays are left alone by the host wrapper."""
    kept = [(None if a is None else np.array(a), None if m is None else np.array(m)) for a, m in models]
    after, results, hit, totals, ms = ctx.models_brush(models, instances, strokes)
    assert ms > 0.0
    same((after, results, hit, totals), want, what)
    for (a, m), (ka, km) in zip(models, kept):
        assert (a is None or (np.asarray(a) == ka).all()) and (m is None or (np.asarray(m) == km).all()), "the wrapper works on copies"
    tensors = _tensors(models)
    results_d, hit_d, totals_d, ms = ctx.models_brush_device(tensors, instances, strokes)
    assert ms > 0.0
    same((_back(tensors), results_d, hit_d, totals_d), want, what + " (device)")
    assert results_d.tobytes() == results.tobytes() and hit_d.tobytes() == hit.tobytes() and totals_d == totals, "the host call is the device call"
    return after, results, hit, totals, tensors


def _check(ctx, name):
    modelbrushcases.property_of(name)
    models, instances, strokes = modelbrushcases.case(name)
    want = modelbrushcases.answer(name)
    return _both(ctx, models, instances, strokes, want, name), want


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [f"column {h}" for h in modelbrushcases.COLUMNS] + ["tall box", "lanes", "misses"])
def test_step_edges(ctx, name):
    _check(ctx, name)


@pytest.mark.parametrize("name", [f"map {m}" for m in modelbrushcases.MAPS] + ["negative"])
def test_maps(ctx, name):
    _check(ctx, name)


@pytest.mark.parametrize("name", ["paint carve paint", "paint paint", "carve", "two instances", "same voxel"])
def test_folds(ctx, name):
    _check(ctx, name)


def test_models_with_a_mask_alone_colours_alone_and_both(ctx):
    _check(ctx, "kinds")


@pytest.mark.parametrize("name", [f"shape {s}" for s in modelbrushcases.SHAPES])
def test_shapes_through_a_rotated_body(ctx, name):
    _check(ctx, name)


@pytest.mark.parametrize("name", ["far", "near miss"])
def test_nothing_hit(ctx, name):
    (after, results, hit, totals, _), _ = _check(ctx, name)
    models = modelbrushcases.case(name)[0]
    assert after[0][0].tobytes() == np.asarray(models[0][0], dtype=np.uint32).tobytes() and totals["carved"] == totals["painted"] == 0
    assert results[0]["voxels"] > 0 and results[0]["sum"].any() and results[0]["moment"].any() and (results[0]["max"] > results[0]["min"]).all()


@pytest.mark.parametrize("name", ["map yaw 30", "shape capsule", "two instances"])
def test_the_same_carve_again_carves_nothing(ctx, name):
    models, instances, strokes = modelbrushcases.case(name)
    carves = [s for s in strokes if s["op"] == CARVE]
    first = modelbrushmodel.brush(models, as_dicts(instances), carves)
    assert first[3]["carved"] > 0
    after, results, hit, totals, tensors = _both(ctx, models, instances, carves, first, name + ": the carves alone")
    second = modelbrushmodel.brush(after, as_dicts(instances), carves)
    again, results2, hit2, totals2, tensors2 = _both(ctx, after, instances, carves, second, name + ": the carves again")
    assert totals2["carved"] == 0 and not results2["carved"].any() and not hit2["carved"].any() and totals2["jobs"] == totals["jobs"]
    for (a, m), (b, n) in zip(after, again):
        assert (a is None or a.tobytes() == b.tobytes()) and (m is None or m.tobytes() == n.tobytes()), "the same arrays"
    for name_ in ("voxels", "sum", "moment", "min", "max"):
        assert (results2[name_] == results[name_]).all()
    # ... and in place on the tensors the first device call left
    results3, hit3, totals3, _ = ctx.models_brush_device(tensors, instances, carves)
    same((_back(tensors), results3, hit3, totals3), second, name + ": in place")


@pytest.mark.parametrize("name", ["4096 strokes", "4096 instances", "256 models"])
def test_limits(ctx, name):
    _check(ctx, name)


def test_one_stroke_hitting_all_bodies(ctx):
    """Every body of the 4096 under one box: every instance is hit, every model changes."""
    models, instances, _ = modelbrushcases.case("4096 instances")
    strokes = [box(CARVE, (-1, -1, -1), (200, 40, 200))]
    want = modelbrushmodel.brush(models, as_dicts(instances), strokes)
    assert (want[2]["carved"] > 0).all() and len(want[2]) == 4096 and want[3]["models"] == 3 and not want[1]["voxels"].any()
    _both(ctx, models, instances, strokes, want, "one stroke, 4096 bodies")


# ---- composed with the calls that exist ---------------------------------------------------------------------------------------------------------------

def _stroke_model(stroke):
    """The stroke rasterised on the host into a dense mask over its footprint, and the identity instance that places it there."""
    lo, hi = modelbrushmodel._footprint(stroke)
    grid = np.meshgrid(*[np.arange(lo[i], hi[i], dtype=np.int64) for i in range(3)], indexing="ij")
    inside = modelbrushmodel._holds(stroke, grid)  # (x, y, z)
    return (None, np.ascontiguousarray(inside.transpose(0, 2, 1))), lo, [hi[i] - lo[i] for i in range(3)]


@pytest.mark.parametrize("name", [f"map {m}" for m in modelbrushcases.MAPS] + ["negative", "shape ellipsoid"])
def test_pair_contacts_overlap_is_carved_before_and_nothing_after(ctx, name):
    models, instances, strokes = modelbrushcases.case(name)
    stroke = [s for s in strokes if s["op"] == CARVE][0]
    rastered, lo, size = _stroke_model(stroke)
    placed = list(instances) + [identity_at(lo, size, len(models))]
    before, _, _, _ = ctx.model_contacts(list(models) + [rastered], placed, [(0, len(instances))], capacity=0)
    after, results, hit, totals, _ = ctx.models_brush(models, instances, [stroke])
    assert before["overlap"][0] == hit[0]["carved"] > 0 and results[0]["carved"] > 0
    assert hit[0]["carved"] >= results[0]["carved"], "several d may share an image"
    behind, _, _, _ = ctx.model_contacts(list(after) + [rastered], placed, [(0, len(instances))], capacity=0)
    assert behind["overlap"][0] == 0 and behind["points"][0] == 0


def test_a_lifted_piece_keeps_its_sums_and_its_mass():
    """A cube of the procedural world cut loose by a carved shell, lifted (COPY) and brushed with a stroke that touches nothing."""
    ws = scenes.load_world("proc64")
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        _, solid = ctx.read_voxels((0, 0, 0), ws.dims, want_argb=False)
        column = np.nonzero(solid[32, 32])[0]
        assert len(column) > 0
        lo = [29, max(int(column.max()) - 5, 1), 29]
        hi = [lo[0] + 6, lo[1] + 6, lo[2] + 6]
        shell = []
        for a in range(3):
            for at in (lo[a] - 1, hi[a]):
                s_lo, s_hi = [v - 1 for v in lo], [v + 1 for v in hi]
                s_lo[a], s_hi[a] = at, at + 1
                shell.append(box(CARVE, s_lo, s_hi))
        ctx.brush(shell, 0)
        pieces, summary, argb, mask, _ = ctx.world_lift_pieces([v - 1 for v in lo], [v + 1 for v in hi], gpu.ANCHOR_GROUND, gpu.LIFT_COPY, 0, 16, 4096)
        assert summary["storedPieces"] == len(pieces) >= 1 and pieces["piece"]["voxels"].sum() > 20
        models, instances = [], []
        for i in range(len(pieces)):
            size, a, m = gpu.lifted_model(pieces, i, argb, mask)
            models.append((np.array(a), np.array(m) != 0))
            instances.append(identity_at(pieces[i]["piece"]["min"].tolist(), size, i))
        after, results, hit, totals, _ = ctx.models_brush(models, instances, [sphere(CARVE, (-500, -500, -500), 3), sphere(PAINT, (-600, -500, -500), 3, RED)])
        assert totals == dict(carved=0, painted=0, models=0, jobs=0) and not hit["carved"].any()
        for i, piece in enumerate(pieces):
            assert after[i][0].tobytes() == models[i][0].tobytes() and after[i][1].tobytes() == models[i][1].tobytes()
            r = results[i]
            assert r["voxels"] == piece["piece"]["voxels"] and (r["sum"] == piece["sum"]).all() and (r["moment"] == piece["moment"]).all()
            assert (r["min"] == 0).all() and (r["max"] == piece["piece"]["max"] - piece["piece"]["min"]).all(), "a piece's box is tight"
            centre, inertia = gpu.model_mass(r)
            lifted_centre, lifted_inertia = gpu.lifted_piece_mass(piece)
            assert inertia.tobytes() == lifted_inertia.tobytes(), "the inertia about the centre does not see the translation"
            c = [float(int(s)) / float(int(r["voxels"])) for s in r["sum"]]  # the formula's c_a; centre = (min + c_a) + 0.5
            assert centre.tolist() == [(0.0 + c[a]) + 0.5 for a in range(3)]
            assert lifted_centre.tolist() == [(float(int(piece["piece"]["min"][a])) + c[a]) + 0.5 for a in range(3)]
    finally:
        ctx.close()


def test_a_painted_voxel_shows_in_the_drawn_frame(ctx):
    """After a PAINT the body drawn by cvxv_models_draw carries the new colour word at a pixel whose ray cvxq_model_pick ends on a painted voxel."""
    models, instances, _ = modelbrushcases.case("map tilt")
    centre = (20, 15, 17)
    strokes = [sphere(PAINT, (centre[0], centre[1], centre[2] - 4), 3, BLUE)]  # the side that faces the eye
    after, results, hit, totals, _ = ctx.models_brush(models, instances, strokes)
    assert results[0]["painted"] > 0 and totals["carved"] == 0
    assert not (np.asarray(models[0][0]) == BLUE).any(), "the colour is new"
    view = gpu.draw_view((20.5, 15.5, -30.5), (-0.16, -0.16, 1.0), (0.01, 0.0, 0.0), (0.0, 0.01, 0.0), 32, 32)
    rays = gpu.view_rays(view)
    hits, _ = ctx.model_pick(after, instances, rays["origin"].reshape(-1, 3), rays["direction"].reshape(-1, 3), rays["maxT"].ravel())
    hits = hits.reshape(32, 32)
    painted = np.argwhere((hits["instance"] == 0) & (hits["argb"] == BLUE))
    assert len(painted) > 0, "a ray ends on a painted voxel"
    y, x = painted[len(painted) // 2]
    s = hits[y, x]["modelVoxel"]
    assert after[0][0][s[0], s[2], s[1]] == BLUE and np.asarray(models[0][0])[s[0], s[2], s[1]] != BLUE
    image, _, ids, _, _ = ctx.models_draw(after, instances, view)
    assert image[y, x] == BLUE and ids[y, x] == 0
    before, _, _, _, _ = ctx.models_draw(models, instances, view)
    assert before[y, x] != BLUE and before[y, x] == np.asarray(models[0][0])[s[0], s[2], s[1]], "the same pixel showed the voxel's old colour word"
