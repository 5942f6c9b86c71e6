"""GPU: first-hit rays against placed voxel models (cvxq_model_pick[_device], include/cpuvox_gpu_model_pick.h).

A call is made on a context through both entry points and, independently, through the host build of the rules (tests/model_pick_rules.cpp, which
runs the sequential pair rule AND the wave's walk and fails where they differ): the bytes must be equal on EVERY ray.  On the rays the numpy
model (tests/modelpickmodel.py) calls unambiguous the device also equals the model.  The scenes are those tests/test_model_pick_cpu.py
builds, plus the ones only the launch can get wrong: more jobs than the walk has waves, one ray, one instance, the most rays, a pair count
that is no multiple of 64.  All but two tests run on a context with nothing uploaded: the calls need no world."""
import numpy as np
import pytest
import torch

import contactsmodel
import modelpickmodel
import pickmodel
import ruleslib
from cpuvox_amd import gpu
from test_gpu_world_contacts import _device_models
from test_gpu_world_dense import _any_world
from test_model_pick_cpu import (FILL, LINE_BODIES, adversarial_scene, assert_adversarial, assert_steps, grid_rays, line_scene, rays_of, run_cases, scene,
                                 steps_scene)
from test_world_contacts_cpu import CUBE, cube_model
from test_world_models_cpu import as_dicts, identity_at, make_instance

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
WORLD_DIMS = (128, 64, 128)  # a world that holds the scene (a world's dimensions are powers of two)
HIT_BYTES = 48


@pytest.fixture(scope="module")
def ctx():
    """A fresh context: no world is ever uploaded into it."""
    context = gpu.Context(0)
    yield context
    context.close()


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("model_pick_rules", tmp_path_factory.mktemp("model_pick_gpu"))


def _host_call(ctx, models, instances, rays):
    hits, ms = ctx.model_pick(models, instances, rays["origin"], rays["direction"], rays["maxT"])
    assert ms > 0.0
    return hits


def _device_call(ctx, models, instances, rays, spare=3):
    """One device call into a sentinel-filled tensor `spare` hits longer than the rays -> the hits; the spare entries must stay as they were."""
    descriptors, keep = _device_models(models)  # noqa: F841  (keep: the tensors the descriptors point to)
    rays_t = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    hits_t = torch.full(((len(rays) + spare) * HIT_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.model_pick_device(descriptors, instances, rays_t, hits_t) > 0.0
    raw = hits_t.cpu().numpy()
    assert (raw[len(rays) * HIT_BYTES:] == SENTINEL).all(), "entries beyond the rays are left alone"
    return raw[:len(rays) * HIT_BYTES].view(gpu.MODEL_HIT_DTYPE)


def _check(ctx, rules, tmp_path, case, what, device=True):
    """Both entry points against the rules program, byte for byte on every ray; returns the hits."""
    models, instances, rays = case
    want, jobs = run_cases(rules, tmp_path, [case])[0]
    got = _host_call(ctx, models, instances, rays)
    differ = np.nonzero((got.view(np.uint8).reshape(-1, HIT_BYTES) != want.view(np.uint8).reshape(-1, HIT_BYTES)).any(axis=1))[0]
    assert len(differ) == 0, f"{what}: {len(differ)} of {len(rays)} rays differ from the rules; first #{differ[0]}: got {got[differ[0]]}, want {want[differ[0]]}"
    if device:
        assert _device_call(ctx, models, instances, rays).tobytes() == want.tobytes(), what + " (device)"
    return got, jobs


# ---- 1. a cube, by hand ------------------------------------------------------------------------------------------------------------------------------

def test_a_cube_by_hand(ctx):
    """The 4 x 4 x 4 cube at (10, 10, 10): six axis rays."""
    models, instances = [cube_model()], [identity_at((10, 10, 10), CUBE, 0, FILL)]
    rays = rays_of([(5, 11.5, 12.5), (20, 11.5, 12.5), (11.5, 2, 12.5), (11.5, 30, 12.5), (11.5, 12.5, 0), (11.5, 12.5, 15.5)],
                   [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -2, 0), (0, 0, 1), (0, 0, -0.5)], 100)
    hits = _host_call(ctx, models, instances, rays)
    assert hits["voxel"].tolist() == [[10, 11, 12], [13, 11, 12], [11, 10, 12], [11, 13, 12], [11, 12, 10], [11, 12, 13]]
    assert hits["face"].tolist() == [0, 1, 2, 3, 4, 5] and hits["t"].tolist() == [5.0, 6.0, 8.0, 8.0, 10.0, 3.0]
    assert hits["instance"].tolist() == [0] * 6 and hits["modelVoxel"].tolist() == [[0, 1, 2], [3, 1, 2], [1, 0, 2], [1, 3, 2], [1, 2, 0], [1, 2, 3]]
    assert (hits["argb"] == 0xFF112233).all() and (hits["pad_"] == 0).all()
    assert _device_call(ctx, models, instances, rays).tobytes() == hits.tobytes()


# ---- 2. the scenes of the CPU test -----------------------------------------------------------------------------------------------------------------

def test_the_scene(ctx, rules, tmp_path):
    models, instances, rays, model = scene()
    got, jobs = _check(ctx, rules, tmp_path, (models, instances, rays), "scene")
    assert jobs > len(rays) and modelpickmodel.compare(got, model, "scene") >= 0.99


def test_adversarial_rays(ctx, rules, tmp_path):
    got, _ = _check(ctx, rules, tmp_path, adversarial_scene(), "adversarial")
    assert_adversarial(got)
    models, instances, _, _ = scene()
    _check(ctx, rules, tmp_path, (models, instances, grid_rays()), "grid")


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1, -1])
def test_the_steps_of_the_walk(ctx, rules, tmp_path, axis, sign):
    s = steps_scene(axis, sign)
    got, _ = _check(ctx, rules, tmp_path, s[:3], f"steps {axis} {sign}")
    assert_steps(s, got)


def test_the_ray_rule(ctx, rules, tmp_path):
    got, _ = _check(ctx, rules, tmp_path, line_scene(twice=True), "line")
    assert got["instance"].tolist() == [2 * k if k >= 0 else -1 for k in LINE_BODIES]


# ---- 3. the launch's limits --------------------------------------------------------------------------------------------------------------------------

def test_more_jobs_than_the_walk_has_waves(ctx, rules, tmp_path):
    """300 rays along a row of 300 boxes, every ray through every box: 90 000 jobs for the 32 768 waves of the walk, which take them in turn.
    Most bodies are air; sixty of them, all along the row, have one of the 16 (y, z) cells set, so that rays end all along the row."""
    rng = np.random.default_rng(9)
    models = [(np.zeros((2, 4, 4), dtype=np.uint32), None)]
    for cell in range(16):
        argb = np.zeros((2, 4, 4), dtype=np.uint32)
        argb[:, cell % 4, cell // 4] = 0xFF000100 + cell
        models.append((argb, None))
    chosen = dict(zip(rng.choice(300, 60, replace=False).tolist(), (1 + rng.integers(0, 16, 60)).tolist()))
    instances = [identity_at((2 * k, 0, 0), (2, 4, 4), chosen.get(k, 0), FILL) for k in range(300)]
    up = np.arange(300) % 2 == 0
    o = np.stack([np.where(up, -3.0, 603.0), rng.uniform(0.05, 3.95, 300), rng.uniform(0.05, 3.95, 300)], axis=-1)
    rays = rays_of(o, np.stack([np.where(up, 1.0, -1.0), np.zeros(300), np.zeros(300)], axis=-1), 1e4)
    got, jobs = _check(ctx, rules, tmp_path, (models, instances, rays), "row")
    assert jobs == 90000 > 32768
    hit = got["instance"][got["instance"] >= 0]
    assert len(hit) > 250 and hit.max() - hit.min() > 200 and len(set(hit.tolist())) > 16


def test_one_ray_one_instance_and_a_ragged_pair_count(ctx, rules, tmp_path):
    models, instances, rays, _ = scene()
    for n_instances, n_rays in ((8, 1), (1, 64), (1, 1), (5, 7), (3, 43)):
        assert n_instances * n_rays in (8, 64, 1, 35, 129)
        _check(ctx, rules, tmp_path, (models, instances[:n_instances], rays[2048:2048 + n_rays]), f"{n_instances} x {n_rays}")


def test_the_most_rays_against_a_one_voxel_model(ctx, rules, tmp_path):
    models = [(np.full((1, 1, 1), 0xFF010203, dtype=np.uint32), None)]
    instances = [make_instance(np.eye(3, dtype=np.int64) << 16, [-5 << 16, -6 << 16, -7 << 16], [3, 4, 5], [8, 9, 10], 0, FILL)]
    rng = np.random.default_rng(3)
    n = gpu.MODEL_PICK_MAX_RAYS
    o = rng.uniform(-4, 16, size=(n, 3))
    rays = rays_of(o, np.array([5.5, 6.5, 7.5]) + rng.uniform(-1.5, 1.5, size=(n, 3)) - o, 1e4)
    got, jobs = _check(ctx, rules, tmp_path, (models, instances, rays), "65536 rays", device=False)
    share = (got["instance"] == 0).mean()
    assert 0.05 < share < 0.6 and jobs > n // 2 and (got["voxel"][got["instance"] == 0] == [5, 6, 7]).all()


# ---- 4. it equals stamping -------------------------------------------------------------------------------------------------------------------------

def test_it_equals_a_fill_and_a_world_pick(ctx):
    """FILL one instance into an empty world that holds its box; cvx_world_pick gives the same voxel, face and argb, and t within 1e-5, on the rays
    that both models -- this call's over the box, pickmodel's over the world -- call unambiguous."""
    models, instances, rays, _ = scene()
    inst = instances[1]  # the ball under a yaw of 30 degrees
    assert all(0 <= inst.boxMin[a] and inst.boxMax[a] <= WORLD_DIMS[a] for a in range(3))
    rays = rays[::4]
    want, amb = modelpickmodel.pick_many(models, as_dicts([inst]), rays["origin"], rays["direction"], rays["maxT"])
    solid = np.zeros(WORLD_DIMS, dtype=bool)
    lo = list(inst.boxMin)
    body = contactsmodel.body(models, as_dicts([inst])[0])
    solid[lo[0]:lo[0] + body.shape[0], lo[1]:lo[1] + body.shape[1], lo[2]:lo[2] + body.shape[2]] = body
    amb |= pickmodel.pick_many(solid, np.zeros(WORLD_DIMS, dtype=np.uint32), rays["origin"], rays["direction"], rays["maxT"])[4]
    assert (~amb).mean() >= 0.99 and (want["instance"][~amb] == 0).mean() > 0.1
    got = _host_call(ctx, models, [inst], rays)
    modelpickmodel.compare(got, (want, amb), "one instance")
    empty = _any_world(WORLD_DIMS, np.zeros(WORLD_DIMS, dtype=bool), np.zeros(WORLD_DIMS, dtype=np.uint32))
    world = gpu.Context(0)
    try:
        world.upload_world(empty)
        world.place_models(models, [inst], 0)
        voxel, face, argb, t = world.pick(rays["origin"], rays["direction"], rays["maxT"])
    finally:
        world.close()
        empty.close()
    ok = ~amb
    assert (voxel[ok] == got["voxel"][ok]).all() and (face[ok] == got["face"][ok]).all() and (argb[ok] == got["argb"][ok]).all()
    assert np.allclose(t[ok].astype(np.float64), got["t"][ok].astype(np.float64), rtol=1e-5, atol=1e-5)


# ---- 5. no world is needed, and none is touched ----------------------------------------------------------------------------------------------------

def test_a_context_with_a_world_gives_the_same_bytes_and_keeps_its_world(ctx):
    models, instances, rays, _ = scene()
    rays = rays[::8]  # (512 of both halves of the scene's rays: some 40 % of them hit)
    mine = _host_call(ctx, models, instances, rays)
    rng = np.random.default_rng(1)
    solid = rng.random(WORLD_DIMS) < 0.2
    colour = np.where(solid, rng.integers(1, 1 << 32, WORLD_DIMS, dtype=np.uint64), 0).astype(np.uint32)
    ws = _any_world(WORLD_DIMS, solid, colour)
    world = gpu.Context(0)
    try:
        world.upload_world(ws)
        before = world.read_voxels((0, 0, 0), WORLD_DIMS)
        theirs = _host_call(world, models, instances, rays)
        device = _device_call(world, models, instances, rays)
        after = world.read_voxels((0, 0, 0), WORLD_DIMS)
    finally:
        world.close()
        ws.close()
    assert theirs.tobytes() == mine.tobytes() == device.tobytes() and (mine["instance"] >= 0).sum() > 100
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[1].any()


# ---- 6. determinism and errors ---------------------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_gives_the_same_bytes(ctx):
    models, instances, rays, _ = scene()
    first, second = _host_call(ctx, models, instances, rays), _host_call(ctx, models, instances, rays)
    assert first.tobytes() == second.tobytes() and (first["instance"] >= 0).sum() > 1000
    assert _device_call(ctx, models, instances, rays).tobytes() == _device_call(ctx, models, instances, rays).tobytes() == first.tobytes()


def test_errors_leave_the_host_array_alone_and_set_the_message(ctx):
    models, instances = [cube_model()], [identity_at((10, 10, 10), CUBE, 0, FILL), identity_at((20, 10, 10), CUBE, 0, FILL)]
    descriptors, keep = gpu.Context._models(models, "test")  # noqa: F841
    inst = gpu.Context._instances(instances)
    rays = rays_of([(5, 11.5, 12.5), (30, 11.5, 12.5)], [(1, 0, 0), (-1, 0, 0)], 100)
    hits = np.full(2 * HIT_BYTES, SENTINEL, dtype=np.uint8)

    def raw(entry=None, models_ptr=True, model_count=1, instance_list=inst, rays_ptr=True, ray_count=2, hits_ptr=True):
        ms = gpu.C.c_float()
        ctx._check((entry or gpu.lib().cvxq_model_pick)(ctx._h, gpu.C.addressof(descriptors) if models_ptr else None, model_count, gpu.C.addressof(instance_list),
                                                        len(instance_list), rays.ctypes.data if rays_ptr else None, ray_count, hits.ctypes.data if hits_ptr else None,
                                                        gpu.C.byref(ms)))

    far = identity_at((10, 13, 10), CUBE, 0, FILL)
    far.boxMax[2] = (1 << 30) + 1
    big_m = identity_at((10, 13, 10), CUBE, 0, FILL)
    big_m.toModel.m[0][0] = (1 << 24) + 1
    for kwargs, message in (
            (dict(models_ptr=False), "cvxq_model_pick: models NULL or modelCount 1"), (dict(model_count=257), "modelCount 257 outside 1 .. 256"),
            (dict(instance_list=gpu.Context._instances([instances[0], identity_at((0, 0, 0), CUBE, 3, FILL)])), "instance 1: model 3 outside 0 .. 0"),
            (dict(instance_list=gpu.Context._instances([far, instances[1]])), r"instance 0: the box \[10, 1073741825\) on axis 2 has a coordinate beyond 2\^30"),
            (dict(instance_list=gpu.Context._instances([instances[0], big_m])), r"instance 1: toModel: m\[0\]\[0\]"),
            (dict(rays_ptr=False), "cvxq_model_pick: rays is NULL"), (dict(hits_ptr=False), "hits is NULL"), (dict(ray_count=0), "rayCount 0 outside 1 .. 65536"),
            (dict(ray_count=65537), "rayCount 65537 outside 1 .. 65536"),
            (dict(entry=gpu.lib().cvxq_model_pick_device, ray_count=-2), "cvxq_model_pick_device: rayCount -2 outside")):
        with pytest.raises(gpu.CvxError, match=message):
            raw(**kwargs)
        assert (hits == SENTINEL).all(), message
    with pytest.raises(gpu.CvxError, match="model 0: argb and solid are both NULL"):
        ctx.model_pick_device([(CUBE, 0, 0)], instances, torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(2 * HIT_BYTES, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="at least 2 x 48 bytes"):
        ctx.model_pick_device([(CUBE, 0, 0)], instances, torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(HIT_BYTES, dtype=torch.uint8, device="cuda"))
    raw()  # the same array takes a good call
    got = hits.view(gpu.MODEL_HIT_DTYPE)
    assert got["voxel"].tolist() == [[10, 11, 12], [23, 11, 12]] and got["instance"].tolist() == [0, 1] and got["t"].tolist() == [5.0, 6.0]
