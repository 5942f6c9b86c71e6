"""GPU: the flight loop with a brush in it, on one context and one world (the world, the poses and the strokes of tests/limitmodels.py's and
tests/limitflight.py's flight sections; tests/test_limit_flight_cpu.py checks them on the CPU): carve the necks of three pillars, lift the three
loose heads into one argb pool and one mask pool on the device, brush them IN PLACE on tensor views of the pools -- one mask begins at an odd
byte --, then sweep them against the world and against each other, test, pick and draw them from the lifted descriptors of the same pools, twice
over; brush again, sweep the free poses down, place them and test them against the new world.

References: tests/modelbrushmodel.py, tests/sweepmodel.py, tests/pairsweepmodel.py, tests/paircontactsmodel.py (byte for byte: integers), the
host builds of the pick rules and the draw rules (byte for byte on every ray and pixel), all on the brushed host copies of the pools."""
import numpy as np
import pytest
import torch

import limitflight as F
import limitmodels as L
import ruleslib
from cpuvox_amd import gpu
from test_gpu_model_draw import _same as same_frame
from test_gpu_model_pick import HIT_BYTES
from test_gpu_model_sequences import _lifted, flight  # noqa: F401  (the fixture: a world, a stroke and three lifted pieces, this module's own)
from test_model_brush_cpu import same as same_brush
from test_model_contacts_cpu import model_of
from test_model_contacts_cpu import same as same_contacts
from test_model_draw_cpu import WORLD
from test_model_sweep_cpu import same as same_pairs
from test_world_models_cpu import as_dicts
from test_world_sweep_cpu import same as same_sweep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return (ruleslib.build("model_pick_rules", tmp_path_factory.mktemp("flight_pick_gpu")), ruleslib.build("model_draw_rules", tmp_path_factory.mktemp("flight_draw_gpu")))


def _views(f):
    """The three pieces as models_brush_device takes them: tensor views (X, Z, Y) into the middle of the two pools."""
    out = []
    for p in f.pieces:
        size = [int(p["piece"]["max"][a]) - int(p["piece"]["min"][a]) for a in range(3)]
        at, n = int(p["offset"]), size[0] * size[1] * size[2]
        out.append((f.argb[at:at + n].view(size[0], size[2], size[1]), f.mask[at:at + n].view(size[0], size[2], size[1])))
    return out


def _pools(f):
    return f.argb.cpu().numpy().view(np.uint32).copy(), f.mask.cpu().numpy().copy()


def _device_round(ctx, descriptors, instances, rays_t):
    """The five read-only calls in their order, all from the lifted descriptors, into fresh tensors."""
    _, falling = F.flight_velocities(instances)
    pairs, motions = F.flight_pairs(instances)
    box_pairs = gpu.box_pairs(instances)
    view = F.flight_view()
    n = view.width * view.height
    contacts = torch.zeros(len(instances) * 120, dtype=torch.uint8, device="cuda")
    points = torch.zeros(4096 * 24, dtype=torch.uint8, device="cuda")
    pair_contacts = torch.zeros(len(pairs) * 144, dtype=torch.uint8, device="cuda")
    pair_results = torch.zeros(len(box_pairs) * 144, dtype=torch.uint8, device="cuda")
    pair_points = torch.zeros(4096 * 32, dtype=torch.uint8, device="cuda")
    hits = torch.zeros(rays_t.numel() // 32 * HIT_BYTES, dtype=torch.uint8, device="cuda")
    frame = [torch.zeros(n, dtype=torch.int32, device="cuda"), torch.full((n,), float("inf"), dtype=torch.float32, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")]
    torch.cuda.synchronize()
    sweeps, totals, _ = ctx.world_sweep_device(descriptors, instances, falling, contacts, points, L.SOLID_OUTSIDE)
    pair_sweeps, pair_totals, _ = ctx.model_sweep_device(descriptors, instances, pairs, motions, pair_contacts)
    contact_totals, _ = ctx.model_contacts_device(descriptors, instances, box_pairs, pair_results, pair_points)
    assert ctx.model_pick_device(descriptors, instances, rays_t, hits) > 0.0
    drawn, _ = ctx.models_draw_device(descriptors, instances, view, WORLD, *frame)
    listed = points.cpu().numpy().view(gpu.CONTACT_POINT_DTYPE)[:totals["points"]]
    pair_listed = pair_points.cpu().numpy().view(gpu.PAIR_POINT_DTYPE)[:contact_totals["points"]]
    return ((sweeps, contacts.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE), listed, totals),
            (pair_sweeps, pair_contacts.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE), pair_totals),
            (pair_results.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE), pair_listed, contact_totals),
            hits.cpu().numpy().view(gpu.MODEL_HIT_DTYPE),
            (*[t.cpu().numpy().view(d).reshape(view.height, view.width) for t, d in zip(frame, (np.uint32, np.float32, np.int32))], drawn))


def _bytes(answer):
    out = []
    for part in answer:
        for item in (part if isinstance(part, tuple) else (part,)):
            out.append(item.tobytes() if hasattr(item, "tobytes") else item)
    return out


def test_a_brush_in_place_on_lifted_pools_is_seen_by_every_call_after_it(flight, rules, tmp_path):  # noqa: F811
    world, ctx = flight.world, flight.world.ctx
    # 1, 2: the necks are carved and the heads lifted (the fixture); one mask begins at an odd byte
    assert len(flight.pieces) == 3 and (flight.pieces["offset"].astype(np.int64) % 2 == 1).any(), flight.pieces["offset"].tolist()
    order, descriptors, before_models = _lifted(flight)
    argb_before, mask_before = _pools(flight)
    levels = [ctx.read_level(k) for k in range(L.FLIGHT_LEVELS + 1)]
    stats = ctx.edit_stats()
    # 3: the brush, in place
    chosen, strokes = F.flight_brush(order)
    want = F.brush_model(before_models, chosen, strokes)
    assert (want[1]["carved"] > 0).all() and want[1]["painted"][order.index("ball")] > 0 and want[3]["models"] == 3
    results, hit, totals, ms = ctx.models_brush_device(_views(flight), chosen, strokes)
    assert ms > 0.0
    # 4: the pools are the model's arrays where the pieces lie and what they were everywhere else
    argb_want, mask_want = argb_before.copy(), mask_before.copy()
    for p, (argb, mask) in zip(flight.pieces, want[0]):
        at = int(p["offset"])
        argb_want[at:at + argb.size], mask_want[at:at + mask.size] = argb.ravel(), mask.ravel()
    argb_after, mask_after = _pools(flight)
    assert argb_after.tobytes() == argb_want.tobytes() and mask_after.tobytes() == mask_want.tobytes(), "the pools after the brush"
    assert argb_after.tobytes() != argb_before.tobytes() and mask_after.tobytes() != mask_before.tobytes()
    _, _, after_models = _lifted(flight)
    same_brush((after_models, results, hit, totals), want, "the brush in place on the pools")
    # 5: the five read-only calls from the lifted descriptors of the same pools, twice over
    instances = L.flight_instances(order)
    reference = F.flight_references(after_models, order, *rules, tmp_path)
    rays_t = torch.from_numpy(np.ascontiguousarray(L.flight_rays()).view(np.uint8).copy()).cuda()
    first = _device_round(ctx, descriptors, instances, rays_t)
    second = _device_round(ctx, descriptors, instances, rays_t)
    same_sweep(first[0], reference[0], "the world sweep of the brushed pieces")
    same_pairs(first[1], reference[1], "the pair sweep of the brushed pieces")
    same_contacts(first[2], reference[2], "the pair contacts of the brushed pieces")
    differ = np.nonzero((first[3].view(np.uint8).reshape(-1, HIT_BYTES) != reference[3].view(np.uint8).reshape(-1, HIT_BYTES)).any(axis=1))[0]
    assert len(differ) == 0, f"{len(differ)} rays differ from the rules; first #{differ[0]}: got {first[3][differ[0]]}, want {reference[3][differ[0]]}"
    same_frame(first[4], reference[4], "the frame of the brushed pieces")
    assert _bytes(second) == _bytes(first), "the second round gives the bytes of the first"
    # 6: ... and they see the brush
    F.assert_the_brush_is_seen(F.flight_references(before_models, order, *rules, tmp_path), reference)
    # 7: the same brush again carves nothing and leaves the sums
    results2, hit2, totals2, _ = ctx.models_brush_device(_views(flight), chosen, strokes)
    again = F.brush_model(after_models, chosen, strokes)
    same_brush((_lifted(flight)[2], results2, hit2, totals2), again, "the same brush again")
    assert totals2["carved"] == 0 and not hit2["carved"].any() and all((results2[name] == results[name]).all() for name in ("voxels", "sum", "moment", "min", "max"))
    assert _pools(flight)[0].tobytes() == argb_after.tobytes() and _pools(flight)[1].tobytes() == mask_after.tobytes()
    assert [ctx.read_level(k) for k in range(L.FLIGHT_LEVELS + 1)] == levels and ctx.edit_stats() == stats, "the world is untouched until the place step"
    # 8: the free poses swept down, placed at `free`, and tested against the new world
    pairs = gpu.box_pairs(instances)
    free = L.assert_flight_poses(world.model(before_models, instances), model_of(before_models, instances, pairs), pairs)  # (carving frees no less)
    flying = [instances[k] for k in free]
    down = [(0, -60, 0)] * len(flying)
    sweeps, sweep_totals, _ = ctx.world_sweep_device(descriptors, flying, down, None, None, L.SOLID_OUTSIDE)
    falling = F.world_sweep_model_on(world.solid, world.colour, after_models, flying, down, L.SOLID_OUTSIDE)
    assert sweeps.tobytes() == falling[0].tobytes() and (sweeps["hit"] > 0).all() and sweep_totals["hits"] == len(flying), "every free pose comes down on something"
    placed = [gpu.instance_moved(inst, s["free"]) for inst, s in zip(flying, sweeps)]
    resting = torch.zeros(len(placed) * 120, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.world_contacts_device(descriptors, placed, resting)
    assert not resting.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE)["overlap"].any(), "at `free` nothing overlaps the world"
    assert ctx.place_models_device(descriptors, placed, L.FLIGHT_LEVELS) > 0.0
    ctx.world_contacts_device(descriptors, placed, resting)
    after = resting.cpu().numpy().view(gpu.CONTACT_RESULT_DTYPE)
    voxels = [int(after_models[inst.model][1].sum()) for inst in placed]
    assert after["overlap"].tolist() == voxels == after["voxels"].tolist(), "a placed pose overlaps the world in every voxel of its carved piece"
    assert voxels != [int(before_models[inst.model][1].sum()) for inst in placed]
    assert ctx.edit_stats() != stats
    assert as_dicts(placed)[0]["box_min"][1] < as_dicts(flying)[0]["box_min"][1]
