"""CPU (no GPU needed): the rules behind cvxv_models_draw (cpuvox_amd/csrc/cvx_model_draw.h), compiled for the host through
tests/model_draw_rules.cpp, against the independent numpy model of tests/modeldrawmodel.py.  The program runs the rule per pixel with NO cull
(every instance, no skip) AND the kernel's tile walk (a rectangle per instance, a list per 8 x 8 tile, the skip behind the key) and fails
when they differ in a byte of any pixel or in a count.

- The scene of tests/test_model_pick_cpu.py seen through SCENE_VIEW: at least 0.99 of the pixels are unambiguous to the model, and on those
  the rules equal the model; with a wall of world in front of half of it, and through the depth test.
- cvxv_view_rays against the rule's rays byte for byte; cvxv_view_from_camera against gpu.screen_rays to 1e-6 per direction component (the
  float rounding of 6e-8 plus two double inversions).
- Hand-made frames: the cube, ties, the eye inside a body and behind one, narrow views whose cull widens its rectangles.
- Every argument check with its message, and the same stand-alone program under -fsanitize=address,undefined."""
import functools
import subprocess

import numpy as np
import pytest

import modeldrawmodel
import ruleslib
from cpuvox_amd import gpu, host
from test_model_pick_cpu import FILL, scene
from test_world_contacts_cpu import CUBE, SANITIZE, colour_of, cube_model, volume_columns
from test_world_models_cpu import as_dicts, call_words, identity_at

WORLD, DEPTH_TEST = gpu.DRAW_WORLD, gpu.DRAW_DEPTH_TEST
SCENE_WORLD = (128, 64, 128)  # a world around the scene (a device world's dimensions are powers of two)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("model_draw_rules", tmp_path_factory.mktemp("model_draw"))


# ---- building cases (the GPU test uses these too) -----------------------------------------------------------------------------------------------

def view_words(view):
    return np.frombuffer(bytes(view), dtype=np.int32)


def case_words(models, instances, view, flags=0, world=None, buffers=None, repeat=0):
    """One case of tests/model_draw_rules.cpp: world = (solid, colour) volumes (x, y, z) or None, buffers = (image, depth, ids) or None."""
    parts = [[int(world is not None)]]
    if world is not None:
        solid, colour = world
        parts += [ruleslib.world_words(solid.shape[1], solid.shape[0], solid.shape[2], 1, volume_columns(solid, colour)), [int(repeat)]]
    parts += [call_words(models, instances), view_words(view), [int(flags)], [int(buffers is not None)]]
    if buffers is not None:
        image, depth, ids = buffers
        parts += [np.ascontiguousarray(image, dtype=np.uint32).view(np.int32).ravel(), np.ascontiguousarray(depth, dtype=np.float32).view(np.int32).ravel(),
                  np.ascontiguousarray(ids, dtype=np.int32).ravel()]
    return parts


def run_cases(rules, tmp_path, cases):
    """[dict(models, instances, view, flags, world, buffers, repeat)] -> [(image, depth, ids, summary dict)]: the program fails when the tile walk
    differs from the un-culled rule."""
    parts = [p for case in cases for p in case_words(**case)]
    raw = ruleslib.run_cases(rules, "cases", tmp_path, *parts, dtype=np.uint8)
    out, at = [], 0
    for case in cases:
        h, w = case["view"].height, case["view"].width
        n = 4 * w * h
        image, depth, ids = raw[at:at + n].view(np.uint32), raw[at + n:at + 2 * n].view(np.float32), raw[at + 2 * n:at + 3 * n].view(np.int32)
        summary = raw[at + 3 * n:at + 3 * n + 32].view(np.int64)
        out.append((image.reshape(h, w).copy(), depth.reshape(h, w).copy(), ids.reshape(h, w).copy(),
                    {"pixelsDrawn": int(summary[0]), "pixelsOccluded": int(summary[1]), "jobs": int(summary[2])}))
        assert summary[3] == 0
        at += 3 * n + 32
    assert at == len(raw)
    return out


def looking_along_z(eye, width, height, half_width, half_height, max_t=1e4, skew=(0.0, 0.0)):
    """A view from `eye` towards +z: at distance 1 the image spans 2 half_width x 2 half_height; skew tilts the image plane a little."""
    dx, dy = 2.0 * half_width / width, 2.0 * half_height / height
    return gpu.draw_view(eye, (-half_width + 0.5 * dx, -half_height + 0.5 * dy, 1.0), (dx, 0.0, skew[0] * dx), (0.0, dy, skew[1] * dy), width, height, max_t)


# the scene's eight instances lie in x 0 .. 60, y -5 .. 34, z 15 .. 60: the whole of it, off every symmetry
SCENE_VIEW = looking_along_z((30.3, 14.7, -38.2), 64, 64, 0.52, 0.42, skew=(0.03, -0.02))


def wall_world():
    """SCENE_WORLD with ground below y = 3 and a wall across z = 18 .. 20 for x < 30, up to y = 40: it hides the left half of the scene's bodies
    and lies in front of some, behind others."""
    solid = np.zeros(SCENE_WORLD, dtype=bool)
    solid[:, :3, :] = True
    solid[:30, :40, 18:20] = True
    return solid, colour_of(solid)


@functools.lru_cache(maxsize=None)
def scene_model(flags=0):
    """The numpy model's frame of the scene through SCENE_VIEW (with the wall world under DRAW_WORLD)."""
    models, instances, _, _ = scene()
    return modeldrawmodel.draw(models, as_dicts(instances), SCENE_VIEW, flags, wall_world() if flags & WORLD else None)


def scene_case(flags=0):
    models, instances, _, _ = scene()
    return dict(models=models, instances=instances, view=SCENE_VIEW, flags=flags, world=wall_world() if flags & WORLD else None)


def one_cube(at=(10, 10, 10)):
    return [cube_model()], [identity_at(at, CUBE, 0, FILL)]


def cube_view(width=20, height=13):
    """An axis-aligned view of the cube at (10, 10, 10) from 12 voxels before it, a pixel a quarter voxel: the centre pixel looks along +z at
    (12.125, 12.125)."""
    step = 0.25 / 12.0
    return gpu.draw_view((12.125, 12.125, -2.0), (-(width // 2) * step, -(height // 2) * step, 1.0), (step, 0, 0), (0, step, 0), width, height, 100.0)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------------

def test_the_scene_view_is_unambiguous_and_covers_the_scene():
    image, depth, ids, amb, counts = scene_model()
    assert 1 - amb.mean() >= 0.99
    assert set(ids.ravel().tolist()) == set(range(-1, 8)), "every body shows somewhere, and so does the background"
    assert 0.2 <= (ids >= 0).mean() <= 0.9


def test_rules_match_the_model_on_the_scene(rules, tmp_path):
    got = run_cases(rules, tmp_path, [scene_case()])[0]
    assert modeldrawmodel.compare(got[:3], scene_model(), "scene") >= 0.99
    assert got[3]["pixelsOccluded"] == 0 and got[3]["pixelsDrawn"] == int((got[2] >= 0).sum()) and got[3]["jobs"] > got[3]["pixelsDrawn"]
    assert (got[0][got[2] < 0] == 0).all() and np.isinf(got[1][got[2] < 0]).all(), "the pixels nothing shows in keep what they held"


def test_rules_match_the_model_behind_the_wall(rules, tmp_path):
    model = scene_model(WORLD)
    assert 1 - model[3].mean() >= 0.99 and model[4]["pixelsOccluded"] > 100 and model[4]["pixelsDrawn"] > 100
    got = run_cases(rules, tmp_path, [scene_case(WORLD)])[0]
    assert modeldrawmodel.compare(got[:3], model, "wall") >= 0.99
    plain = run_cases(rules, tmp_path, [scene_case()])[0]
    assert got[3]["pixelsDrawn"] + got[3]["pixelsOccluded"] == plain[3]["pixelsDrawn"] and got[3]["jobs"] == plain[3]["jobs"]


def test_two_calls_through_the_depth_test_equal_one(rules, tmp_path):
    models, instances, _, _ = scene()
    whole = run_cases(rules, tmp_path, [scene_case()])[0]
    first = run_cases(rules, tmp_path, [dict(models=models, instances=instances[:3], view=SCENE_VIEW)])[0]
    marked = first[2] - 1000  # (the ids the first call wrote, told apart from the second call's)
    second = run_cases(rules, tmp_path, [dict(models=models, instances=instances[3:], view=SCENE_VIEW, flags=DEPTH_TEST, buffers=(first[0], first[1], marked))])[0]
    ids = np.where(second[2] >= 0, second[2] + 3, second[2] + 1000)
    # a body of each list at exactly the same t: the one call gives it to the lower index, the second of two calls takes it (its ray ends AT the depth)
    tie = (second[2] >= 0) & (first[2] >= 0) & (second[1] == first[1])
    assert tie.sum() < 40 and (whole[2][tie] == first[2][tie]).all()
    keep = ~tie
    assert (ids[keep] == whole[2][keep]).all() and second[0][keep].tobytes() == whole[0][keep].tobytes() and second[1].tobytes() == whole[1].tobytes()
    assert (second[2] >= 0).sum() > 100 and (second[2] < -1).sum() > 100, "both calls show in the frame"
    # a NaN or negative depth leaves the pixel alone
    depth = np.full((64, 64), np.inf, dtype=np.float32)
    depth[:, :20], depth[:, 20:40] = np.nan, -1.0
    image, ids0 = np.full((64, 64), 0xABCD, dtype=np.uint32), np.full((64, 64), -7, dtype=np.int32)
    got = run_cases(rules, tmp_path, [dict(models=models, instances=instances, view=SCENE_VIEW, flags=DEPTH_TEST, buffers=(image, depth, ids0))])[0]
    assert (got[0][:, :40] == 0xABCD).all() and (got[2][:, :40] == -7).all() and got[1][:, :40].tobytes() == depth[:, :40].tobytes()
    right = whole[2][:, 40:]
    assert (got[2][:, 40:][right >= 0] == right[right >= 0]).all() and (got[2][:, 40:][right < 0] == -7).all()


def test_a_cube_by_hand(rules, tmp_path):
    models, instances = one_cube()
    view = cube_view()
    image, depth, ids, summary = run_cases(rules, tmp_path, [dict(models=models, instances=instances, view=view)])[0]
    assert ids[6, 10] == 0 and depth[6, 10] == 12.0 and image[6, 10] == 0xFF112233, "the centre pixel looks along +z from z = -2 at the face z = 10"
    # the cube spans x 10 .. 14 at 12 voxels: pixels whose centre lies within (-2.125 .. 1.875) / 0.25 steps of the middle one
    shown = ids >= 0
    assert shown[6].tolist() == [bool(-2.125 < 0.25 * (x - 10) < 1.875) for x in range(20)]
    assert summary["pixelsDrawn"] == int(shown.sum()) and summary["jobs"] == summary["pixelsDrawn"] and summary["pixelsOccluded"] == 0
    assert (image[~shown] == 0).all() and (ids[~shown] == -1).all()


def test_view_rays_are_the_rules_rays(rules, tmp_path):
    degenerate = gpu.draw_view((1, 2, 3), (0, 0, 0), (1, 0, 0), (0, 1, 0), 5, 3, 7.0)  # (pixel (0, 0) has no direction)
    windows = [(SCENE_VIEW, 0, 0, 64, 64), (SCENE_VIEW, 13, 7, 5, 3), (cube_view(), 0, 0, 20, 13), (degenerate, 0, 0, 5, 3)]
    parts = [p for view, *window in windows for p in (view_words(view), window)]
    raw = ruleslib.run_cases(rules, "rays", tmp_path, *parts, dtype=np.uint8)
    at = 0
    for view, x0, y0, w, h in windows:
        rays = gpu.view_rays(view, x0, y0, w, h)
        assert rays.shape == (h, w) and rays.tobytes() == raw[at:at + 32 * w * h].tobytes()
        at += 32 * w * h
    assert at == len(raw)
    whole = gpu.view_rays(SCENE_VIEW)
    assert whole[7:10, 13:18].tobytes() == gpu.view_rays(SCENE_VIEW, 13, 7, 5, 3).tobytes()
    first = gpu.view_rays(degenerate)[0, 0]
    assert first["direction"].tolist() == [0, 0, 0] and first["maxT"] == -1.0 and gpu.view_rays(degenerate)[0, 1]["maxT"] == 7.0
    # ... and the model's rays, from numpy's own arithmetic, to a float's rounding
    o, d, good = modeldrawmodel.view_rays(SCENE_VIEW)
    assert good.all() and np.abs(whole["direction"] - d).max() <= 2 ** -23 and (whole["origin"] == o).all() and (whole["maxT"] == SCENE_VIEW.maxT).all()
    with pytest.raises(ValueError, match="view_rays"):
        gpu.view_rays(SCENE_VIEW, 60, 0, 5, 1)


@pytest.mark.parametrize("pose", [((64.0, 40.0, 26.0), (35.0, 20.0, 0.0)), ((-20.0, 70.0, 150.0), (-15.0, 200.0, 0.0)), ((30.0, 10.0, 30.0), (0.01, 45.0, 0.0))])
def test_view_from_camera_gives_screen_rays(pose):
    width, height = 48, 36
    p = host.camera_pose(list(pose[0]), pose[1], width, height)
    lods, far = host.setup_lods(p, 128, width, height, 1.0)
    camera = host.setup_frame(p, lods, far, width, height, 64, True).camera
    view = gpu.view_from_camera(camera, width, height, 500.0)
    assert (view.width, view.height, view.maxT) == (width, height, 500.0)
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    o, d = gpu.screen_rays(camera, width, height, px.ravel(), py.ravel())
    rays = gpu.view_rays(view).ravel()
    assert np.abs(rays["direction"].astype(np.float64) - d).max() <= 1e-6
    assert (rays["origin"] == o.astype(np.float32)).all() and (rays["maxT"] == 500.0).all()
    with pytest.raises(ValueError, match="view_from_camera"):
        gpu.view_from_camera(camera, 0, height)


def hand_cases():
    """Frames only a rule can get wrong, by name."""
    cube, at = cube_model(), (10, 10, 10)
    models, one = one_cube()
    view = cube_view(24, 24)
    cases = {}
    # exactly tied bodies: the same cube three times, and a second cube beside it at the same distance
    cases["ties"] = dict(models=models, instances=[identity_at(at, CUBE, 0, FILL)] * 3 + [identity_at((6, 10, 10), CUBE, 0, FILL)], view=view)
    # the eye inside a body (face 6, t = 0) and inside a box beside its body
    cases["inside"] = dict(models=models, instances=one, view=gpu.draw_view((11.5, 11.5, 11.5), (-0.5, -0.5, 1.0), (0.1, 0, 0), (0, 0.1, 0), 10, 10, 50.0))
    # a body wholly behind the eye, and one across the eye plane
    back = gpu.draw_view((12.0, 12.0, 30.0), (-0.5, -0.5, 1.0), (0.1, 0, 0), (0, 0.1, 0), 10, 10, 50.0)
    cases["behind"] = dict(models=models, instances=one, view=back)
    cases["across"] = dict(models=[(np.full((4, 40, 4), 0xFF00FF00, dtype=np.uint32), None)], instances=[identity_at((10, 10, 10), (4, 4, 40), 0, FILL)], view=back)
    # a sub-pixel body far away
    far = gpu.draw_view((0.5, 0.5, -2000.0), (-0.16, -0.16, 1.0), (0.02, 0, 0), (0, 0.02, 0), 17, 17, 1e4)
    cases["speck"] = dict(models=[(np.full((1, 1, 1), 0xFF123456, dtype=np.uint32), None)], instances=[identity_at((0, 0, 0), (1, 1, 1), 0, FILL)], view=far)
    # a narrow view: a pixel is 2e-8 of the distance, less than the float rounding of a direction turns the ray, and the cull widens
    narrow = gpu.draw_view((13.3, 13.7, -1000.0), (-32 * 2e-8, -32 * 2e-8, 1.0), (2e-8, 0, 0), (0, 2e-8, 0), 64, 64, 1e4)
    cases["narrow"] = dict(models=models, instances=[identity_at((12, 12, 10), CUBE, 0, FILL), identity_at((8, 8, 30), CUBE, 0, FILL)], view=narrow)
    # 1 x 1 and a single row
    cases["1x1"] = dict(models=models, instances=one, view=gpu.draw_view((12.5, 12.5, 0.0), (0, 0, 1), (0.01, 0, 0), (0, 0.01, 0), 1, 1, 50.0))
    cases["row"] = dict(models=models, instances=one, view=gpu.draw_view((12.5, 12.5, 0.0), (-1.0, 0.0, 1.0), (2.0 / 300, 0, 0), (0, 0.01, 0), 300, 1, 50.0))
    # a far limit that ends the rays of the outer pixels before the cube
    cases["maxT"] = dict(models=models, instances=one, view=cube_view(24, 24))
    cases["maxT"]["view"].maxT = 12.2
    return cases


def test_hand_made_frames(rules, tmp_path):
    cases = hand_cases()
    got = dict(zip(cases, run_cases(rules, tmp_path, list(cases.values()))))
    image, depth, ids, summary = got["ties"]
    assert set(ids.ravel().tolist()) == {-1, 0, 3}, "of identical instances the lowest index shows"
    image, depth, ids, summary = got["inside"]
    assert (ids == 0).all() and (depth == 0.0).all() and summary["pixelsDrawn"] == 100
    assert got["behind"][3] == {"pixelsDrawn": 0, "pixelsOccluded": 0, "jobs": 0}
    assert got["across"][3]["pixelsDrawn"] > 0 and got["across"][1][got["across"][2] >= 0].min() == 0.0
    assert got["speck"][3]["pixelsDrawn"] == 1 and got["speck"][2][8, 8] == 0
    assert got["narrow"][3]["pixelsDrawn"] == 64 * 64 and set(got["narrow"][2].ravel().tolist()) == {0}
    assert got["1x1"][3] == {"pixelsDrawn": 1, "pixelsOccluded": 0, "jobs": 1} and got["1x1"][1][0, 0] == 10.0
    assert 0 < got["row"][3]["pixelsDrawn"] < 300
    assert 0 < got["maxT"][3]["pixelsDrawn"] < 256 and got["maxT"][1][got["maxT"][2] >= 0].max() <= 12.2


def test_the_cull_leaves_instances_out_and_widens_in_narrow_views(rules, tmp_path):
    """(What the program prints of the cull: the rule has no cull, so nothing else shows it.)"""
    cases = hand_cases()
    parts = [p for name in ("speck", "narrow") for p in case_words(**cases[name])] + [p for p in case_words(**scene_case())]
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    src.write_bytes(b"".join(np.asarray(p, dtype=np.int64).astype(np.int32).tobytes() for p in parts))
    lines = subprocess.check_output([rules, "cases", str(src), str(dst)], text=True).splitlines()
    grow = [int(line.split("grow ")[1].split(",")[0]) for line in lines]
    listed = [(int(line.split(", ")[1].split(" ")[0]), int(line.rsplit(" ", 1)[1])) for line in lines]
    assert grow[0] == 1 and grow[2] == 1 and grow[1] > 1, lines
    assert listed[0][0] < listed[0][1] / 2 and listed[2][0] < listed[2][1], lines


MESSAGES = [
    ("models NULL or modelCount 1 outside 1 .. 256", -1), ("instances NULL or instanceCount 4097 outside 1 .. 4096", -1), ("model 0: argb and solid are both NULL", -1),
    ("instance 0: the box [0, 0) on axis 1 is empty", -1), ("view is NULL", -1), ("view 8193 x 4 outside 1 .. 8192", -1), ("view 4 x 0 outside 1 .. 8192", -1),
    ("view maxT -1 is negative or NaN", -1), ("view maxT nan is negative or NaN", -1), ("view origin, dir0, dirX or dirY is not finite on axis 2", -1),
    ("view origin, dir0, dirX or dirY is not finite on axis 1", -1), ("view: the matrix [dirX dirY dir0] is singular", -1), ("view: the matrix [dirX dirY dir0] is singular", -1),
    ("flags 0x4 has unknown bits", -1), ("image, depth and ids are all NULL", -1), ("CVXV_DRAW_DEPTH_TEST without depth", -1),
]


def _check_args(text):
    lines = text.splitlines()
    assert lines[:2] == ["-1", "-1"], "without a context"
    at = 2
    for message, code in MESSAGES:
        assert lines[at] == f"{code} cvxv_models_draw: {message}" and lines[at + 1] == f"{code} cvxv_models_draw_device: {message}", (lines[at], message)
        at += 2
    assert lines[at] == lines[at + 1] == "-3 world LOD 0 has not been uploaded", "DRAW_WORLD without a world: cvx_world_pick's error"
    assert lines[at + 2:] == ["-1 -1 -1 -1 -1 0", "-1 -1 -1 -1"]


def test_calls_fail_cleanly_with_their_messages(rules):
    """(The program itself fails when an error wrote to a host array or the summary.)"""
    _check_args(subprocess.check_output([rules, "args"], text=True))


def test_python_wrappers_check_their_arguments():
    ctx = object.__new__(gpu.Context)
    models, instances = one_cube()
    with pytest.raises(ValueError, match="models_draw: a model is a pair"):
        ctx.models_draw([np.zeros((2, 2, 2), dtype=np.uint32)], instances, cube_view())
    with pytest.raises(ValueError, match="models_draw: view is a gpu.DrawView"):
        ctx.models_draw(models, instances, None)
    with pytest.raises(ValueError, match=r"models_draw: depth has the shape \(height, width\)"):
        ctx.models_draw(models, instances, cube_view(), depth=np.zeros((20, 13), dtype=np.float32))
    with pytest.raises(ValueError, match="models_draw_device: a model is"):
        ctx.models_draw_device([(1, 2)], instances, cube_view(), 0, None)
    assert gpu.DRAW_VIEW_DTYPE.itemsize == 96 and gpu.DRAW_SUMMARY_DTYPE.itemsize == 32 and (gpu.DRAW_WORLD, gpu.DRAW_DEPTH_TEST) == (1, 2)


def test_the_rules_run_clean_under_the_sanitizers(rules, tmp_path):
    """The same program built stand-alone (its own main, nothing of the library linked, nothing loaded into Python) with
    -fsanitize=address,undefined: the hand-made frames, the cube behind the wall and the scene's rays run to the end and give the bytes of the
    plain build."""
    program = ruleslib.build("model_draw_rules", tmp_path, *SANITIZE, "-DMODEL_DRAW_RULES_NO_LIBRARY", link_library=False)
    models, instances = one_cube((40, 6, 24))
    walled = dict(models=models, instances=instances, view=looking_along_z((30.3, 14.7, -38.2), 24, 24, 0.52, 0.42), flags=WORLD, world=wall_world())
    cases = list(hand_cases().values()) + [walled, dict(walled, repeat=1)]
    plain, clean = tmp_path / "plain", tmp_path / "clean"
    plain.mkdir()
    clean.mkdir()
    for a, b in zip(run_cases(rules, plain, cases), run_cases(program, clean, cases)):
        assert all(a[i].tobytes() == b[i].tobytes() for i in range(3)) and a[3] == b[3]
    parts = [view_words(SCENE_VIEW), [0, 0, 64, 64]]
    assert ruleslib.run_cases(rules, "rays", plain, *parts, dtype=np.uint8).tobytes() == ruleslib.run_cases(program, "rays", clean, *parts, dtype=np.uint8).tobytes()
