"""GPU: the loop the placed-model calls were built for, on one context and one world (the world and the poses of tests/limitmodels.py's flight
section; tests/test_limit_models_cpu.py checks them on the CPU): carve the necks of three pillars, lift the three loose heads into one argb pool
and one mask pool on the device, test a dozen poses of them against the world (cvxc_world_contacts) and against each other
(cvxp_model_contacts), pick them (cvxq_model_pick), all three from the lifted device descriptors -- addresses into the middle of the shared
pools, one of them at an odd byte -- twice over; then place the free poses and pick the new world.

References: tests/contactsmodel.py, tests/paircontactsmodel.py (byte for byte: integers), the host build of the pick rules (byte for byte on
every ray), tests/pickmodel.py and tests/modelpickmodel.py for the world pick after placing."""
import numpy as np
import pytest
import torch

import limitmodels as L
import modelpickmodel
import modelsmodel
import pickmodel
import ruleslib
from cpuvox_amd import gpu
from test_gpu_model_pick import HIT_BYTES
from test_gpu_world_contacts import World
from test_model_contacts_cpu import model_of
from test_model_contacts_cpu import same as same_pairs
from test_model_pick_cpu import run_cases
from test_world_contacts_cpu import same as same_contacts
from test_world_models_cpu import as_dicts

pytestmark = pytest.mark.gpu

POOL = 4096


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("model_pick_rules", tmp_path_factory.mktemp("model_sequences_gpu"))


class Flight:
    """The context after the stroke and the lift, the pools, the lifted descriptors and their read-back arrays."""


@pytest.fixture(scope="module")
def flight():
    solid, colour, neck, pieces = L.flight_world()
    f = Flight()
    f.world = World(L.FLIGHT_DIMS, solid.copy(), colour.copy())
    try:
        ctx = f.world.ctx
        ctx.brush(neck, L.FLIGHT_LEVELS)
        f.argb = torch.zeros(POOL, dtype=torch.int32, device="cuda")
        f.mask = torch.zeros(POOL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        f.pieces, f.summary, _ = ctx.world_lift_pieces_device((0, 0, 0), L.FLIGHT_DIMS, gpu.ANCHOR_GROUND, f.argb, f.mask, gpu.LIFT_REMOVE, L.FLIGHT_LEVELS, 16, POOL)
        f.world.solid, f.world.colour = L.flight_after_lift()  # what the host expects of the stroke and the REMOVE (the calls below are checked against it)
        yield f
    finally:
        f.world.close()


def _lifted(f):
    """(the pieces' names in the device's order, the lifted descriptors, the read-back host models)."""
    pieces = L.flight_world()[3]
    by_min = {tuple(lo): name for name, (lo, _, _, _) in pieces.items()}
    order = [by_min[tuple(p["piece"]["min"].tolist())] for p in f.pieces]
    descriptors = [gpu.lifted_model(f.pieces, i, f.argb.data_ptr(), f.mask.data_ptr()) for i in range(len(f.pieces))]
    argb, mask = f.argb.cpu().numpy().view(np.uint32), f.mask.cpu().numpy()  # the pools, read back once
    host_models = [gpu.lifted_model(f.pieces, i, argb, mask) for i in range(len(f.pieces))]
    return order, descriptors, [(a, m.astype(bool)) for _, a, m in host_models]


def _device_round(ctx, descriptors, instances, pairs, rays_t, capacities):
    """The three calls in their order, all from the lifted descriptors, into fresh tensors -> their bytes and totals."""
    results = torch.zeros(len(instances) * 120, dtype=torch.uint8, device="cuda")
    points = torch.zeros(capacities[0] * 24, dtype=torch.uint8, device="cuda")
    pair_results = torch.zeros(len(pairs) * 144, dtype=torch.uint8, device="cuda")
    pair_points = torch.zeros(capacities[1] * 32, dtype=torch.uint8, device="cuda")
    hits = torch.zeros(rays_t.numel() // 32 * HIT_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    totals, _ = ctx.world_contacts_device(descriptors, instances, results, points)
    pair_totals, _ = ctx.model_contacts_device(descriptors, instances, pairs, pair_results, pair_points)
    assert ctx.model_pick_device(descriptors, instances, rays_t, hits) > 0.0
    return ((results.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE), points.cpu().numpy().view(gpu.CONTACT_POINT_DTYPE), totals),
            (pair_results.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE), pair_points.cpu().numpy().view(gpu.PAIR_POINT_DTYPE), pair_totals),
            hits.cpu().numpy().view(gpu.MODEL_HIT_DTYPE))


def _bytes(answer):
    contacts, pair_contacts, hits = answer
    return (contacts[0].tobytes(), contacts[1].tobytes(), contacts[2], pair_contacts[0].tobytes(), pair_contacts[1].tobytes(), pair_contacts[2], hits.tobytes())


# ---- C1. one context, one world ------------------------------------------------------------------------------------------------------------------

def test_the_three_families_on_lifted_pieces_twice_over(flight, rules, tmp_path):
    world, ctx = flight.world, flight.world.ctx
    pieces = L.flight_world()[3]
    assert len(flight.pieces) == 3 and flight.summary["storedPieces"] == 3 and flight.summary["storedVoxels"] == sum(p[1][0] * p[1][1] * p[1][2] for p in pieces.values()) <= POOL
    offsets = flight.pieces["offset"].astype(np.int64)
    assert (offsets % 2 == 1).any(), f"a piece's mask starts at an odd byte of the pool (offsets {offsets.tolist()})"
    order, descriptors, host_models = _lifted(flight)
    assert sorted(order) == sorted(pieces)
    for name, (argb, mask) in zip(order, host_models):
        assert argb.tobytes() == pieces[name][2].tobytes() and mask.tobytes() == pieces[name][3].tobytes(), f"the lifted {name} is the piece the host cuts out"
    instances = L.flight_instances(order)
    pairs = gpu.box_pairs(instances)
    want_world = world.model(host_models, instances)
    want_pairs = model_of(host_models, instances, pairs)
    free = L.assert_flight_poses(want_world, want_pairs, pairs)
    rays = L.flight_rays()
    want_hits, jobs = run_cases(rules, tmp_path, [(host_models, instances, rays)])[0]
    assert jobs > len(rays) and (want_hits["instance"] >= 0).sum() > 100 and len(set(want_hits["instance"].tolist())) > 8
    model = modelpickmodel.pick_many(host_models, as_dicts(instances), rays["origin"], rays["direction"], rays["maxT"])
    assert modelpickmodel.compare(want_hits, model, "the rules against the model") >= 0.9
    levels = [ctx.read_level(k) for k in range(L.FLIGHT_LEVELS + 1)]
    stats = ctx.edit_stats()
    rays_t = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).cuda()
    capacities = (want_world[2]["points"], want_pairs[2]["points"])
    assert min(capacities) > 0
    first = _device_round(ctx, descriptors, instances, pairs, rays_t, capacities)
    second = _device_round(ctx, descriptors, instances, pairs, rays_t, capacities)
    same_contacts(first[0], want_world, "world contacts of the lifted pieces")
    same_pairs(first[1], want_pairs, "pair contacts of the lifted pieces")
    differ = np.nonzero((first[2].view(np.uint8).reshape(-1, HIT_BYTES) != want_hits.view(np.uint8).reshape(-1, HIT_BYTES)).any(axis=1))[0]
    assert len(differ) == 0, f"{len(differ)} rays differ from the rules; first #{differ[0]}: got {first[2][differ[0]]}, want {want_hits[differ[0]]}"
    assert _bytes(second) == _bytes(first), "the second round gives the bytes of the first"
    # the host forms, given the read-back arrays
    results, points, totals, _ = ctx.world_contacts(host_models, instances)
    pair_results, pair_points, pair_totals, _ = ctx.model_contacts(host_models, instances, pairs)
    hits, _ = ctx.model_pick(host_models, instances, rays["origin"], rays["direction"], rays["maxT"])
    assert _bytes(((results, points, totals), (pair_results, pair_points, pair_totals), hits)) == _bytes(first), "the host forms give the same bytes"
    assert [ctx.read_level(k) for k in range(L.FLIGHT_LEVELS + 1)] == levels and ctx.edit_stats() == stats, "the calls write nothing"
    assert len(free) >= 3


# ---- C2. the same context goes on ----------------------------------------------------------------------------------------------------------------

def test_placing_the_free_poses_and_picking_the_new_world(flight):
    world, ctx = flight.world, flight.world.ctx
    order, descriptors, host_models = _lifted(flight)
    instances = L.flight_instances(order)
    pairs = gpu.box_pairs(instances)
    free = L.assert_flight_poses(world.model(host_models, instances), model_of(host_models, instances, pairs), pairs)
    placed = [instances[k] for k in free]
    assert all(inst.op == gpu.BRUSH_FILL for inst in placed)
    rays = L.flight_rays()
    o, d, max_t = rays["origin"], rays["direction"], rays["maxT"]
    before = ctx.pick(o, d, max_t)
    bodies, _ = ctx.model_pick(host_models, placed, o, d, max_t)
    world_model = pickmodel.pick_many(world.solid, world.colour, o, d, max_t)
    body_model = modelpickmodel.pick_many(host_models, as_dicts(placed), o, d, max_t)
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    both = (world_model[1] >= 0) & (body_model[0]["instance"] >= 0)
    close = both & (np.abs(world_model[3] - body_model[0]["t"]) * length < pickmodel.EPS)  # (the two sources' hits at one place: either may be the nearer)
    ok = ~(world_model[4] | body_model[1] | close)
    print(f"placing: {ok.mean():.4f} of the {len(rays)} rays are unambiguous to both models")
    assert ok.mean() >= 0.9
    before_hits = np.zeros(len(rays), dtype=gpu.PICK_HIT_DTYPE)
    before_hits["voxel"], before_hits["face"], before_hits["argb"], before_hits["t"] = before
    pickmodel.compare_picks(before_hits, world_model, "the world pick before placing")
    modelpickmodel.compare(bodies, body_model, "the pick of the placed poses")
    assert ctx.place_models_device(descriptors, placed, L.FLIGHT_LEVELS) > 0.0
    voxels = [int(host_models[inst.model][1].sum()) for inst in placed]
    results, _, totals, _ = ctx.world_contacts(host_models, placed)
    assert results["overlap"].tolist() == voxels == results["voxels"].tolist() and totals["overlap"] == sum(voxels), "a placed pose overlaps the world in every voxel of its piece"
    device_results = torch.zeros(len(placed) * 120, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.world_contacts_device(descriptors, placed, device_results)
    assert device_results.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE).tobytes() == results.tobytes()
    solid, colour = modelsmodel.place(world.solid, world.colour, host_models, as_dicts(placed))  # the host's world with the poses filled in
    assert solid.sum() == world.solid.sum() + sum(voxels)
    voxel, face, argb, t = ctx.pick(o, d, max_t)
    from_bodies = (bodies["instance"] >= 0) & ((before[1] < 0) | (bodies["t"] < before[3]))
    want_voxel = np.where(from_bodies[:, None], bodies["voxel"], before[0])
    want_face, want_argb = np.where(from_bodies, bodies["face"], before[1]), np.where(from_bodies, bodies["argb"], before[2])
    want_t = np.where(from_bodies, bodies["t"], before[3])
    assert (from_bodies & ok).sum() > 20 and (~from_bodies & (before[1] >= 0) & ok).sum() > 20, "both sources win somewhere"
    assert (voxel[ok] == want_voxel[ok]).all() and (face[ok] == want_face[ok]).all() and (argb[ok] == want_argb[ok]).all()
    assert np.allclose(t[ok].astype(np.float64), want_t[ok].astype(np.float64), rtol=1e-5, atol=1e-5)
    after_model = pickmodel.pick_many(solid, colour, o, d, max_t)  # and the new world's own model agrees where it is sure
    sure = ok & ~after_model[4]
    assert (voxel[sure] == after_model[0][sure]).all() and (face[sure] == after_model[1][sure]).all() and (argb[sure] == after_model[2][sure]).all()
