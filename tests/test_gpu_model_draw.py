"""GPU: placed voxel models drawn into a view (cvxv_models_draw[_device], include/cpuvox_gpu_model_draw.h).

A call is made on a context through both entry points and, independently, through the host build of the rules (tests/model_draw_rules.cpp, which
runs the rule per pixel with no cull AND the kernel's tile walk and fails where they differ): image, depth, ids and the summary must be equal
byte for byte on EVERY pixel.  On the pixels the numpy model (tests/modeldrawmodel.py) calls unambiguous the device also equals the model, and
the same frame composed from the shipped calls (view_rays -> model_pick -> pick) equals it byte for byte.  The scenes are those
tests/test_model_draw_cpu.py builds, plus the ones only the launch can get wrong.  Unless a world is needed the context has nothing uploaded."""
import numpy as np
import pytest
import torch

import modeldrawmodel
import pickmodel
import ruleslib
import scenes
from cpuvox_amd import gpu
from test_gpu_world_contacts import World, _device_models
from test_model_draw_cpu import (DEPTH_TEST, SCENE_VIEW, SCENE_WORLD, WORLD, cube_view, hand_cases, looking_along_z, one_cube, run_cases, scene_case, scene_model,
                                 wall_world)
from test_model_pick_cpu import FILL, scene
from test_world_contacts_cpu import CUBE, colour_of
from test_world_models_cpu import identity_at

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SPARE = 5


@pytest.fixture(scope="module")
def ctx():
    """A fresh context: no world is ever uploaded into it."""
    context = gpu.Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("model_draw_rules", tmp_path_factory.mktemp("model_draw_gpu"))


@pytest.fixture(scope="module")
def walled():
    """The wall world of the CPU test in a context of its own."""
    w = World(SCENE_WORLD, *wall_world())
    yield w
    w.close()


def _buffers(case):
    """The arrays a case starts from (the rules program's defaults where it names none)."""
    h, w = case["view"].height, case["view"].width
    if case.get("buffers") is not None:
        return tuple(np.array(a, dtype=t).reshape(h, w) for a, t in zip(case["buffers"], (np.uint32, np.float32, np.int32)))
    return np.zeros((h, w), dtype=np.uint32), np.full((h, w), np.inf, dtype=np.float32), np.full((h, w), -1, dtype=np.int32)


def _host_call(ctx, case):
    image, depth, ids = _buffers(case)
    image, depth, ids, summary, ms = ctx.models_draw(case["models"], case["instances"], case["view"], case.get("flags", 0), image, depth, ids)
    assert ms > 0.0
    return image, depth, ids, summary


def _device_call(ctx, case, want_none=()):
    """One device call into tensors SPARE elements longer than the image, the spare ones a sentinel that must stay."""
    descriptors, keep = _device_models(case["models"])  # noqa: F841  (keep: the tensors the descriptors point to)
    n = case["view"].width * case["view"].height
    tensors = []
    for k, start in enumerate(_buffers(case)):
        if k in want_none:
            tensors.append(None)
            continue
        t = torch.full((n + SPARE,), SENTINEL, dtype=torch.int32, device="cuda")
        t[:n] = torch.from_numpy(start.view(np.int32).ravel().copy()).cuda()
        tensors.append(t)
    torch.cuda.synchronize()
    summary, ms = ctx.models_draw_device(descriptors, case["instances"], case["view"], case.get("flags", 0), *tensors)
    assert ms > 0.0
    out = []
    for t, dtype in zip(tensors, (np.uint32, np.float32, np.int32)):
        if t is None:
            out.append(None)
            continue
        raw = t.cpu().numpy()
        assert (raw[n:] == SENTINEL).all(), "elements behind the image are left alone"
        out.append(raw[:n].view(dtype).reshape(case["view"].height, case["view"].width))
    return (*out, summary)


def _same(got, want, what):
    for name, a, b in zip(("image", "depth", "ids"), got[:3], want[:3]):
        differ = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
        assert len(differ) == 0, (f"{what}: {len(differ)} pixels differ from the rules in {name}; first (x {differ[0][1]}, y {differ[0][0]}): got {a[tuple(differ[0])]}, "
                                  f"want {b[tuple(differ[0])]}")
    assert got[3] == want[3], f"{what}: summary {got[3]} vs the rules' {want[3]}"


def _check(ctx, rules, tmp_path, case, what, device=True):
    """Both entry points against the rules program, byte for byte on every pixel; returns the rules' frame."""
    want = run_cases(rules, tmp_path, [case])[0]
    _same(_host_call(ctx, case), want, what)
    if device:
        _same(_device_call(ctx, case), want, what + " (device)")
    return want


# ---- 1. a cube, by hand ------------------------------------------------------------------------------------------------------------------------------

def test_a_cube_by_hand(ctx):
    """The 4^3 cube at (10, 10, 10) through an axis-aligned 20 x 13 view (partial tiles on both axes), over sentinels in all three arrays."""
    models, instances = one_cube()
    start = (np.full((13, 20), 0xABCDEF01, dtype=np.uint32), np.full((13, 20), 77.5, dtype=np.float32), np.full((13, 20), -9, dtype=np.int32))
    case = dict(models=models, instances=instances, view=cube_view(), buffers=start)
    image, depth, ids, summary = _host_call(ctx, case)
    assert ids[6, 10] == 0 and depth[6, 10] == 12.0 and image[6, 10] == 0xFF112233, "the centre pixel looks along +z from z = -2 at the face z = 10"
    shown = np.zeros((13, 20), dtype=bool)
    shown[:, 2:18] = True  # the cube spans 16 pixels of a quarter voxel around the middle column, and every row
    assert (ids[shown] == 0).all() and (image[shown] == 0xFF112233).all() and (depth[shown] >= 12.0).all() and (depth[shown] < 12.3).all()
    assert (ids[~shown] == -9).all() and (image[~shown] == 0xABCDEF01).all() and (depth[~shown] == 77.5).all(), "untouched pixels keep the sentinels"
    assert summary == {"pixelsDrawn": 16 * 13, "pixelsOccluded": 0, "jobs": 16 * 13}
    got = _device_call(ctx, case)
    assert all(got[i].tobytes() == (image, depth, ids)[i].tobytes() for i in range(3)) and got[3] == summary
    # any of the three may be left out
    only_ids = _device_call(ctx, case, want_none=(0, 1))
    assert only_ids[0] is None and only_ids[1] is None and only_ids[2].tobytes() == ids.tobytes() and only_ids[3] == summary


# ---- 2. the scene of the CPU test ------------------------------------------------------------------------------------------------------------------

def test_the_scene(ctx, rules, tmp_path):
    want = _check(ctx, rules, tmp_path, scene_case(), "scene")
    got = _host_call(ctx, scene_case())
    assert modeldrawmodel.compare(got[:3], scene_model(), "scene") >= 0.99 and want[3]["pixelsDrawn"] > 1000


# ---- 3. the same frame through the shipped calls ---------------------------------------------------------------------------------------------------

def _composed(world_ctx, case):
    """view_rays -> model_pick -> pick up to the body's t, composed in numpy: (image, depth, ids, pixelsDrawn, pixelsOccluded)."""
    image, depth, ids = _buffers(case)
    rays = gpu.view_rays(case["view"]).ravel()
    hits, _ = world_ctx.model_pick(case["models"], case["instances"], rays["origin"], rays["direction"], rays["maxT"])
    hit = hits["instance"] >= 0
    shows = hit.copy()
    if case.get("flags", 0) & WORLD:
        _, face, _, _ = world_ctx.pick(rays["origin"][hit], rays["direction"][hit], hits["t"][hit])
        shows[np.nonzero(hit)[0][face >= 0]] = False
    shows = shows.reshape(ids.shape)
    image[shows], depth[shows], ids[shows] = hits["argb"].reshape(ids.shape)[shows], hits["t"].reshape(ids.shape)[shows], hits["instance"].reshape(ids.shape)[shows]
    return image, depth, ids, int(shows.sum()), int(hit.sum() - shows.sum())


def test_the_frame_equals_the_shipped_calls_composed(rules, tmp_path):
    solid, colour = wall_world()
    world = World(SCENE_WORLD, solid.copy(), colour.copy())
    try:
        edit = [{"op": gpu.BRUSH_CARVE, "shape": 0, "a": (8, 10, 16), "b": (22, 30, 22), "argb": 0},
                {"op": gpu.BRUSH_FILL, "shape": 1, "a": (44, 16, 14), "b": (5, 0, 0), "argb": 0xFF334455}]
        world.ctx.brush(edit, 5)
        pickmodel.apply_strokes(world.solid, world.colour, edit)
        for flags in (0, WORLD):
            case = dict(scene_case(), flags=flags, world=(world.solid, world.colour) if flags else None)
            got = _host_call(world.ctx, case)
            image, depth, ids, drawn, occluded = _composed(world.ctx, case)
            assert got[0].tobytes() == image.tobytes() and got[1].tobytes() == depth.tobytes() and got[2].tobytes() == ids.tobytes(), flags
            assert (got[3]["pixelsDrawn"], got[3]["pixelsOccluded"]) == (drawn, occluded)
            assert occluded > 100 if flags else occluded == 0
            _same(got, run_cases(rules, tmp_path, [case])[0], f"edited world, flags {flags}")
    finally:
        world.close()


# ---- 4. the ray rule ----------------------------------------------------------------------------------------------------------------------------------

def test_the_ray_rule(ctx, rules, tmp_path):
    """Overlapping and exactly tied bodies; permuting the list changes ids through the permutation alone, and a tie goes to the lower index."""
    models, instances, _, _ = scene()
    plain = _check(ctx, rules, tmp_path, scene_case(), "scene")
    order = [5, 2, 7, 0, 3, 6, 1, 4]
    permuted = _host_call(ctx, dict(scene_case(), instances=[instances[k] for k in order]))
    back = np.array(order + [-1])[permuted[2]]  # (the last entry: ids of -1)
    assert permuted[0].tobytes() == plain[0].tobytes() and permuted[1].tobytes() == plain[1].tobytes() and (back == plain[2]).all()
    ties = hand_cases()["ties"]
    want = _check(ctx, rules, tmp_path, ties, "ties")
    assert set(want[2].ravel().tolist()) == {-1, 0, 3}
    swapped = _host_call(ctx, dict(ties, instances=ties["instances"][::-1]))
    assert set(swapped[2].ravel().tolist()) == {-1, 0, 1} and swapped[1].tobytes() == want[1].tobytes(), "the cube listed three times shows as the lowest of its indices"


# ---- 5. occlusion ------------------------------------------------------------------------------------------------------------------------------------

def test_occlusion_by_the_world(walled, rules, tmp_path):
    """The wall stands in front of the left half of the scene's bodies and behind others; the ground lies behind all of them."""
    world = (walled.solid, walled.colour)
    hidden = _check(walled.ctx, rules, tmp_path, scene_case(WORLD), "behind the wall")
    plain = _check(walled.ctx, rules, tmp_path, scene_case(), "flag off: the wall is ignored", device=False)
    assert hidden[3]["pixelsOccluded"] > 100 and plain[3]["pixelsOccluded"] == 0
    assert hidden[3]["pixelsDrawn"] + hidden[3]["pixelsOccluded"] == plain[3]["pixelsDrawn"]
    seen = hidden[2] >= 0
    assert (hidden[2][seen] == plain[2][seen]).all() and seen[:, 40:].sum() > 100 and (plain[2][:, :20] >= 0).sum() > (hidden[2][:, :20] >= 0).sum()
    assert modeldrawmodel.compare(_host_call(walled.ctx, scene_case(WORLD))[:3], scene_model(WORLD), "wall") >= 0.99
    _, _, _, drawn, occluded = _composed(walled.ctx, scene_case(WORLD))
    assert (drawn, occluded) == (hidden[3]["pixelsDrawn"], hidden[3]["pixelsOccluded"])
    # repeat mode: from a tile further back the eye sees the scene through the nearer tile's wall too
    far = looking_along_z((30.3, 14.7, -166.2), 64, 64, 0.2, 0.16, skew=(0.03, -0.02))
    bounded = _check(walled.ctx, rules, tmp_path, dict(scene_case(WORLD), view=far), "from afar", device=False)
    walled.ctx.set_world_repeat(True)
    try:
        repeated = _check(walled.ctx, rules, tmp_path, dict(scene_case(WORLD), view=far, repeat=1, world=world), "repeating world")
        assert repeated[3]["pixelsOccluded"] > bounded[3]["pixelsOccluded"] > 0
    finally:
        walled.ctx.set_world_repeat(False)


def test_the_world_flag_needs_a_world(ctx):
    with pytest.raises(gpu.CvxError, match="world LOD 0 has not been uploaded"):
        ctx.models_draw(*one_cube(), cube_view(), WORLD)


# ---- 6. the depth test --------------------------------------------------------------------------------------------------------------------------------

def test_two_calls_through_the_depth_test_equal_one(ctx, rules, tmp_path):
    models, instances, _, _ = scene()
    whole = _host_call(ctx, scene_case())
    first = _host_call(ctx, dict(models=models, instances=instances[:3], view=SCENE_VIEW))
    second_case = dict(models=models, instances=instances[3:], view=SCENE_VIEW, flags=DEPTH_TEST, buffers=(first[0], first[1], first[2] - 1000))
    second = _check(ctx, rules, tmp_path, second_case, "the second call")
    ids = np.where(second[2] >= 0, second[2] + 3, second[2] + 1000)
    tie = (second[2] >= 0) & (first[2] >= 0) & (second[1] == first[1])  # (a body of each list at the same t: the second call takes it, one call the lower index)
    assert tie.sum() < 40 and (whole[2][tie] == first[2][tie]).all()
    assert (ids[~tie] == whole[2][~tie]).all() and second[0][~tie].tobytes() == whole[0][~tie].tobytes() and second[1].tobytes() == whole[1].tobytes()
    depth = np.full((64, 64), np.inf, dtype=np.float32)
    depth[:, :20], depth[:, 20:40] = np.nan, -1.0
    start = (np.full((64, 64), 0xABCD, dtype=np.uint32), depth, np.full((64, 64), -7, dtype=np.int32))
    got = _check(ctx, rules, tmp_path, dict(scene_case(), flags=DEPTH_TEST, buffers=start), "NaN and negative depths")
    assert (got[0][:, :40] == 0xABCD).all() and (got[2][:, :40] == -7).all() and got[1][:, :40].tobytes() == depth[:, :40].tobytes()
    assert (got[2][:, 40:] >= 0).sum() > 100


# ---- 7. limits the launch can get wrong ---------------------------------------------------------------------------------------------------------------

def test_4096_instances_in_64_by_64(ctx, rules, tmp_path):
    """A body of one voxel to 4^3 per pixel, seen from far away: every tile's list holds its 64 bodies and their neighbours', out of 4096."""
    models = [(np.full((n, n, n), 0xFF000000 + n, dtype=np.uint32), None) for n in (1, 2, 3, 4)]
    instances = [identity_at((5 * (k % 64), 5 * (k // 64), (k * 7) % 11), (k % 4 + 1,) * 3, k % 4, FILL) for k in range(4096)]
    view = gpu.draw_view((160.3, 160.7, -4000.0), (-32 * 5 / 4000, -32 * 5 / 4000, 1.0), (5 / 4000, 0, 0), (0, 5 / 4000, 0), 64, 64, 1e5)
    want = _check(ctx, rules, tmp_path, dict(models=models, instances=instances, view=view), "4096 bodies")
    assert want[3]["pixelsDrawn"] > 3000 and len(set(want[2].ravel().tolist())) > 3000


def test_the_other_limits(ctx, rules, tmp_path):
    cases = hand_cases()
    models, one = one_cube()
    # more instances in a tile than one list step of 64: a hundred cubes one behind the other, the nearest listed last
    cases["queue"] = dict(models=models, instances=[identity_at((10, 10, 10 + 6 * k), CUBE, 0, FILL) for k in range(99, -1, -1)], view=cube_view(24, 24))
    # a rectangle that ends exactly on a tile border: the one-voxel-wide slab spans pixels 1.5 .. 5.9, so its rectangle is x 0 .. 7
    cases["border"] = dict(models=[(np.full((1, 1, 4), 0xFF00AA00, dtype=np.uint32), None)], instances=[identity_at((10, 10, 10), (1, 4, 1), 0, FILL)], view=cube_view(20, 24))
    cases["wide row"] = dict(models=models, instances=one, view=gpu.draw_view((12.5, 12.5, 0.0), (-1.0, 0.0, 1.0), (2.0 / 8192, 0, 0), (0, 0.01, 0), 8192, 1, 50.0))
    got = {name: _check(ctx, rules, tmp_path, case, name) for name, case in cases.items()}
    assert (got["queue"][2][got["queue"][2] >= 0] == 99).all() and got["queue"][3]["jobs"] > 2 * got["queue"][3]["pixelsDrawn"]
    assert got["border"][3]["pixelsDrawn"] > 0 and (got["border"][2][:, 8:] == -1).all()
    assert (got["inside"][1] == 0.0).all() and got["behind"][3] == {"pixelsDrawn": 0, "pixelsOccluded": 0, "jobs": 0}
    assert got["across"][3]["pixelsDrawn"] > 0 and got["speck"][3]["pixelsDrawn"] == 1 and got["1x1"][3]["pixelsDrawn"] == 1
    assert 0 < got["wide row"][3]["pixelsDrawn"] < 8192


def test_errors_leave_the_outputs_alone_and_set_the_message(ctx):
    models, instances = one_cube()
    descriptors, keep = ctx._models(models, "test")  # noqa: F841
    view = cube_view()
    image, depth, ids = np.full((13, 20), 0x11, dtype=np.uint32), np.full((13, 20), 2.5, dtype=np.float32), np.full((13, 20), -3, dtype=np.int32)
    singular = gpu.draw_view((0, 0, 0), (0, 0, 1), (1, 0, 0), (2, 0, 0), 20, 13, 10.0)
    negative = cube_view()
    negative.maxT = -1.0
    for bad_view, flags, pointers, message in [(view, 8, (1, 1, 1), "flags 0x8 has unknown bits"), (view, 0, (0, 0, 0), "image, depth and ids are all NULL"),
                                               (view, DEPTH_TEST, (1, 0, 1), "CVXV_DRAW_DEPTH_TEST without depth"), (singular, 0, (1, 1, 1), "is singular"),
                                               (negative, 0, (1, 1, 1), "maxT -1 is negative or NaN"), (view, WORLD, (1, 1, 1), "world LOD 0 has not been uploaded")]:
        with pytest.raises(gpu.CvxError, match=message):
            ctx._models_draw(gpu.lib().cvxv_models_draw, descriptors, 1, instances, bad_view, flags, *[a.ctypes.data if on else None for a, on in zip((image, depth, ids), pointers)])
    with pytest.raises(gpu.CvxError, match="instanceCount 0 outside"):
        ctx.models_draw(models, [], view)
    assert (image == 0x11).all() and (depth == 2.5).all() and (ids == -3).all()
    assert ctx.models_draw(models, instances, view)[3]["pixelsDrawn"] == 16 * 13, "the context goes on working"


# ---- 8. colour ----------------------------------------------------------------------------------------------------------------------------------------

def test_a_body_shows_the_word_the_blit_shows_for_the_same_voxels():
    """A single-colour body FILLed into a world, rendered and blitted; then CARVEd out and drawn by this call into the blitted empty frame."""
    dims, width, height, argb = (64, 64, 64), 64, 48, 0xFF3C78B4
    solid = np.zeros(dims, dtype=bool)
    solid[:, :4, :] = True
    world = World(dims, solid, colour_of(solid))
    try:
        ctx = world.ctx
        ctx.set_resolution(width, height)
        frame = scenes.make_frame(world.ws, width, height, [32.5, 20.5, 4.5], (12.0, 0.0, 0.0), lod_error=1.0)
        for i in range(6):
            frame.camera.LODDistances[i] = 1e9
        box = {"shape": 0, "a": (26, 10, 30), "b": (38, 22, 34), "argb": argb}
        ctx.brush([dict(box, op=gpu.BRUSH_FILL)], 5)
        ctx.clear_raybuffers(0, 0)
        ctx.draw_segments(frame, 0)
        rendered = ctx.blit_segments(0)
        ctx.brush([dict(box, op=gpu.BRUSH_CARVE)], 5)
        ctx.clear_raybuffers(0, 0)
        ctx.draw_segments(frame, 0)
        empty = torch.zeros(width * height, dtype=torch.int32, device="cuda")
        ids = torch.full((width * height,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ctx.blit_segments_batch(0, 1, empty.data_ptr())
        view = gpu.view_from_camera(frame.camera, width, height, 1e4)
        body = [((12, 12, 4), torch.full((12 * 4 * 12,), argb - (1 << 32), dtype=torch.int32, device="cuda"), None)]
        torch.cuda.synchronize()
        placed = [identity_at((26, 10, 30), (12, 12, 4), 0, FILL)]
        summary, _ = ctx.models_draw_device([(body[0][0], body[0][1].data_ptr(), 0)], placed, view, WORLD, empty, None, ids)
        drawn = empty.cpu().numpy().view(np.uint32).reshape(height, width)
        shown = ids.cpu().numpy().reshape(height, width) == 0
        assert summary["pixelsDrawn"] == shown.sum() > 100 and (rendered == argb).sum() > 100
        # the interior of the large face: pixels all of whose neighbours show the body in both images
        inner = shown & (rendered == argb)
        for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0)):
            inner &= np.roll(shown & (rendered == argb), (dy, dx), axis=(0, 1))
        assert inner.sum() > 50 and (drawn[inner] == rendered[inner]).all() and (drawn[inner] == argb).all()
        assert (drawn[~shown] == ctx.blit_segments(0)[~shown]).all(), "the rest of the frame is the blit's"
        # ... and into the image the blit left in the context
        ctx.blit_segments(0, to_host=False)
        pointer, nbytes = ctx.screen_device_ptr()
        assert nbytes >= 4 * width * height
        again, _ = ctx.models_draw_device([(body[0][0], body[0][1].data_ptr(), 0)], placed, view, WORLD, pointer)
        assert again == summary
    finally:
        world.close()


# ---- 9. from the device pools -------------------------------------------------------------------------------------------------------------------------

def test_lifted_pieces_are_drawn_from_their_pools(rules, tmp_path):
    dims = (32, 64, 32)
    solid = np.zeros(dims, dtype=bool)
    solid[:, :8, :] = True
    solid[10:18, 8:30, 12:20] = True  # a pillar on the ground ...
    solid[8:20, 30:36, 10:22] = True  # ... with a wider head
    neck = [{"op": gpu.BRUSH_CARVE, "shape": 0, "a": (0, 24, 0), "b": (32, 28, 32), "argb": 0}]
    world = World(dims, solid.copy(), colour_of(solid))
    try:
        ctx = world.ctx
        ctx.brush(neck, 5)
        pickmodel.apply_strokes(world.solid, world.colour, neck)
        argb = torch.zeros(4096, dtype=torch.int32, device="cuda")
        mask = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pieces, summary, _ = ctx.world_lift_pieces_device((0, 0, 0), dims, gpu.ANCHOR_GROUND, argb, mask, gpu.LIFT_REMOVE, 5, 16, 4096)
        assert len(pieces) == 1 and summary["storedPieces"] == 1
        lifted = gpu.lifted_model(pieces, 0, argb.data_ptr(), mask.data_ptr())
        size = lifted[0]
        n = size[0] * size[1] * size[2]
        host_model = (argb.cpu().numpy().view(np.uint32)[:n].reshape(size[0], size[2], size[1]), mask.cpu().numpy()[:n].reshape(size[0], size[2], size[1]).astype(bool))
        world.solid[8:20, 28:36, 10:22] &= ~host_model[1].transpose(0, 2, 1)  # the REMOVE
        world.colour[~world.solid] = 0
        instances = [identity_at((8, 40, 10), size, 0, FILL), identity_at((6, 10, 22), size, 0, FILL)]  # in the air, and behind the pillar's stump
        view = looking_along_z((15.7, 24.3, -30.0), 40, 40, 0.45, 0.5, skew=(0.02, 0.01))
        want = run_cases(rules, tmp_path, [dict(models=[host_model], instances=instances, view=view, flags=WORLD, world=(world.solid, world.colour))])[0]
        assert want[3]["pixelsDrawn"] > 50 and set(want[2].ravel().tolist()) == {-1, 0, 1}
        tensors = [torch.zeros(1600, dtype=torch.int32, device="cuda"), torch.full((1600,), float("inf"), dtype=torch.float32, device="cuda"),
                   torch.full((1600,), -1, dtype=torch.int32, device="cuda")]
        torch.cuda.synchronize()
        got, ms = ctx.models_draw_device([lifted], instances, view, WORLD, *tensors)
        frames = [t.cpu().numpy().view(d).reshape(40, 40) for t, d in zip(tensors, (np.uint32, np.float32, np.int32))]
        _same((*frames, got), want, "lifted")
    finally:
        world.close()


def test_the_same_call_twice_gives_the_same_bytes(ctx):
    a, b = _host_call(ctx, scene_case()), _host_call(ctx, scene_case())
    assert all(a[i].tobytes() == b[i].tobytes() for i in range(3)) and a[3] == b[3]
