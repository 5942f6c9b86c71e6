"""GPU: cvxm_pair_sweep / cvxm_pair_sweep_device (include/cpuvox_gpu_pair_sweep.h) three ways: the host call against the numpy model of
tests/pairsweepmodel.py -- sweeps, contacts and summary byte for byte --, the device call into sentinel-filled tensors against the same, and
against the shipped cvxp_model_contacts composed a pose at a time: no overlap at any instance_moved(I_a, o_j) with j < hit (every j on a miss), an
overlap at hit, the contacts' bytes at `at`.  The cases are tests/pairsweepcases.py's, the ones tests/test_model_sweep_cpu.py runs through the host
rules; each first asserts from the model the property it is named for.  Everything is integers: no tolerance."""
import numpy as np
import pytest
import torch

import limitmodels as L
import pairsweepcases
import sweepmodel
from cpuvox_amd import gpu
from test_gpu_model_sequences import _lifted, flight  # noqa: F401  (the fixture: a world, a stroke and three lifted pieces)
from test_gpu_world_contacts import _device_models
from test_model_sweep_cpu import same

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
RESULT_BYTES = 144


def _own(results):
    """The bytes of results without what names the pair and orders the list: what they say of the overlap itself."""
    out = np.array(results, copy=True)
    out["a"] = out["b"] = 0
    out["firstPoint"] = 0
    return out.tobytes()


@pytest.fixture(scope="module")
def ctx():
    """A fresh context: no world is ever uploaded into it."""
    context = gpu.Context(0)
    yield context
    context.close()


def _device_call(ctx, models, instances, pairs, motions, spare=2):
    """One device call into a sentinel-filled tensor -> (sweeps, the tensor's entries, totals)."""
    descriptors, keep = _device_models(models)  # noqa: F841  (keep: the tensors the descriptors point to)
    contacts = torch.full(((len(pairs) + spare) * RESULT_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sweeps, totals, ms = ctx.model_sweep_device(descriptors, instances, pairs, motions, contacts)
    assert ms > 0.0
    alone, totals_alone, _ = ctx.model_sweep_device(descriptors, instances, pairs, motions, None)
    assert alone.tobytes() == sweeps.tobytes() and totals_alone == totals, "contacts NULL: the sweeps alone"
    return sweeps, contacts.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE), totals


def _composed(ctx, models, instances, pairs, motions, sweeps, contacts):
    """The shipped model_contacts on instance_moved(I_a, o_j) against I_b: overlap 0 for every j < hit (every j when hit is -1), an overlap at
    hit with the sweep's contacts.  A pair's answer depends on (a, b, v) alone: equal triples have equal bytes, and one of each is composed."""
    first = {}
    for p, ((a, b), v) in enumerate(zip(np.asarray(pairs).tolist(), np.asarray(motions).tolist())):
        q = first.setdefault((a, b, tuple(v)), p)
        assert sweeps[q]["sweep"].tobytes() == sweeps[p]["sweep"].tobytes() and _own(contacts[q:q + 1]) == _own(contacts[p:p + 1])
    poses = []  # (a, the offset, b, whether it overlaps, the pair when this is its pose `at`)
    for (a, b, v), p in first.items():
        s = sweeps[p]["sweep"]
        path = sweepmodel.path(v)
        assert (list(path[s["hit"]][0]) if s["hit"] >= 0 else list(v)) == s["at"].tolist()
        poses += [(a, o, b, False, -1) for o, _ in path[:s["hit"] if s["hit"] >= 0 else len(path) - 1]]
        poses.append((a, tuple(s["at"].tolist()), b, bool(s["hit"] >= 0), p))
    room = gpu.MODELS_MAX_INSTANCES - len(instances)
    for at in range(0, len(poses), room):
        batch = poses[at:at + room]
        moved = list(instances) + [gpu.instance_moved(instances[a], o) for a, o, _, _, _ in batch]
        results, _, _, _ = ctx.model_contacts(models, moved, [(len(instances) + i, b) for i, (_, _, b, _, _) in enumerate(batch)], capacity=0)
        assert ((results["overlap"] > 0) == np.array([touch for _, _, _, touch, _ in batch])).all(), "a pose before `hit` overlaps, or the pose `hit` does not"
        for i, (_, _, _, _, p) in enumerate(batch):
            if p >= 0:
                assert _own(results[i:i + 1]) == _own(contacts[p:p + 1]), f"pair {p}: the contacts are cvxp_model_contacts' of the pose `at`"
    return len(poses)


def _check(ctx, name):
    pairsweepcases.property_of(name)
    models, instances, pairs, motions = pairsweepcases.case(name)
    want = pairsweepcases.answer(name)
    n = len(pairs)
    sweeps, contacts, totals, ms = ctx.model_sweep(models, instances, pairs, motions)
    assert ms > 0.0
    same((sweeps, contacts, totals), want, name)
    assert _composed(ctx, models, instances, pairs, motions, sweeps, contacts) >= 1
    got = _device_call(ctx, models, instances, pairs, motions)
    same((got[0], got[1][:n], got[2]), want, name + " (device)")
    assert (got[1][n:].view(np.uint8) == SENTINEL).all(), "entries beyond the pairs keep what they held"
    return want


# ---- 1. the thin shell and the ends of the range --------------------------------------------------------------------------------------------------------

def test_a_plate_passing_through_a_plate_is_caught(ctx):
    models, instances, pairs, motions = pairsweepcases.case("thin shell")
    ends = [instances[0], gpu.instance_moved(instances[0], motions[0]), instances[1]]
    results, _, totals, _ = ctx.model_contacts(models, ends, [(0, 2), (1, 2)], capacity=0)
    assert results["overlap"].tolist() == [0, 0] and totals["touching"] == 0, "cvxp_model_contacts sees nothing at either end pose"
    s = _check(ctx, "thin shell")[0]["sweep"][0]
    assert (s["hit"], s["axis"], s["sign"]) == (4, 1, -1)


@pytest.mark.parametrize("name", ["starts overlapping", "hit at n", "miss by one", "still"])
def test_the_ends_of_the_range(ctx, name):
    _check(ctx, name)


# ---- 2. the path ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["-x", "+x", "-y", "+y", "-z", "+z", *pairsweepcases.TIES])
def test_every_axis_and_sign_and_the_tie_order(ctx, name):
    s = _check(ctx, name)[0]["sweep"]
    assert s["hit"][0] == s["hit"][1] > 0, "the hit of (a, b) under v is the hit of (b, a) under -v"


# ---- 3. maps and boxes ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["maps", "boxes"])
def test_maps_and_boxes(ctx, name):
    _check(ctx, name)


# ---- 4. waves ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [f"column {h}" for h in pairsweepcases.HEIGHTS] + ["lane 0", "lane 63", "windows", "later step"])
def test_steps_lanes_and_windows_of_a_wave(ctx, name):
    _check(ctx, name)


# ---- 5. pairs ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [f"{n} pairs" for n in pairsweepcases.COUNTS] + ["repeats"])
def test_every_round_of_the_search_and_the_limit(ctx, name):
    _check(ctx, name)


def test_the_same_call_twice_and_backwards(ctx):
    """The same call twice: the same bytes; the pairs reversed: the same bytes per pair but for firstPoint, the running sum."""
    models, instances, pairs, motions = pairsweepcases.case("4097 pairs")
    want = pairsweepcases.answer("4097 pairs")
    again = ctx.model_sweep(models, instances, pairs, motions)
    assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes() and again[2] == want[2]
    back = ctx.model_sweep(models, instances, pairs[::-1], motions[::-1])
    assert back[0][::-1].tobytes() == want[0].tobytes() and back[2] == want[2]
    mine, theirs = back[1][::-1].copy(), want[1].copy()
    mine["firstPoint"] = theirs["firstPoint"] = 0
    assert mine.tobytes() == theirs.tobytes()


# ---- 6. the long motion and the fuzz ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["long hit", "long miss"])
def test_a_component_of_4096(ctx, name):
    _check(ctx, name)


def test_300_random_pairs(ctx):
    hits = pairsweepcases.answer("fuzz")[0]["sweep"]["hit"]
    assert (hits > 0).mean() >= 0.20 and (hits == -1).mean() >= 0.10 and (hits == 0).mean() >= 0.05, "the model alone: the test cannot pass vacuously"
    _check(ctx, "fuzz")


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------------------------------

def test_errors_set_the_message(ctx):
    models, instances, pairs, motions = pairsweepcases.case("thin shell")
    with pytest.raises(gpu.CvxError, match="cvxm_pair_sweep: pair 0: motion 4097 on axis 1 beyond 4096"):
        ctx.model_sweep(models, instances, pairs, [(0, 4097, 0)])
    with pytest.raises(gpu.CvxError, match=r"cvxm_pair_sweep: pair 0: \(1, 1\) pairs an instance with itself"):
        ctx.model_sweep(models, instances, [(1, 1)], motions)
    _check(ctx, "hit at n")  # the context goes on


# ---- 8. the flight loop -----------------------------------------------------------------------------------------------------------------------------------

def test_lifted_pieces_swept_against_their_neighbours(flight):  # noqa: F811
    """Carve, lift, and sweep: every pose of the lifted pieces heads for the middle of them all, the pairs are cvxp_box_pairs' with the largest
    velocity component as the margin (two boxes widened by it meet wherever v_a - v_b can bring them together), each in both orders, and the
    motion of a pair is v_a - v_b.  Body a moved by `free` does not overlap b wherever the pair was free at the start; moved by `at` it does
    wherever the sweep hit."""
    ctx = flight.world.ctx
    order, descriptors, host_models = _lifted(flight)
    instances = L.flight_instances(order)
    centres = np.array([[(i.boxMin[c] + i.boxMax[c]) / 2 for c in range(3)] for i in instances])
    velocity = np.rint((centres.mean(axis=0) - centres) * 0.8).astype(np.int64)
    pairs = gpu.box_pairs(instances, margin=int(np.abs(velocity).max()))
    pairs = np.concatenate([pairs, pairs[:, ::-1]])
    motions = velocity[pairs[:, 0]] - velocity[pairs[:, 1]]
    assert len(pairs) >= 40 and np.abs(motions).max() <= gpu.SWEEP_MAX_MOTION
    contacts = torch.zeros(len(pairs) * RESULT_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sweeps, totals, ms = ctx.model_sweep_device(descriptors, instances, pairs, motions, contacts)
    contacts = contacts.cpu().numpy().view(gpu.PAIR_RESULT_DTYPE)
    hit = sweeps["sweep"]["hit"]
    assert ms > 0.0 and (hit > 0).sum() >= 6 and (hit == -1).sum() >= 6 and (hit == 0).sum() >= 2 and totals["hits"] == (hit >= 0).sum(), hit.tolist()
    half = len(pairs) // 2
    assert hit[:half].tolist() == hit[half:].tolist(), "(b, a) under v_b - v_a"
    host = ctx.model_sweep(host_models, instances, pairs, motions)
    assert host[0].tobytes() == sweeps.tobytes() and host[1].tobytes() == contacts.tobytes() and host[2] == totals, "the host form gives the same bytes"
    n = len(instances)
    rest = list(instances) + [gpu.instance_moved(instances[a], s["free"]) for (a, _), s in zip(pairs, sweeps["sweep"])]
    further = list(instances) + [gpu.instance_moved(instances[a], s["at"]) for (a, _), s in zip(pairs, sweeps["sweep"])]
    moved_pairs = [(n + p, int(b)) for p, (_, b) in enumerate(pairs)]
    free = ctx.model_contacts(host_models, rest, moved_pairs, capacity=0)[0]
    assert not free["overlap"][hit != 0].any(), "moved by `free`, no pair that was free at the start overlaps"
    assert (free["overlap"][hit == 0] > 0).all(), "the pairs that started overlapping still do: their `free` is no motion"
    touching = ctx.model_contacts(host_models, further, moved_pairs, capacity=0)[0]
    assert ((touching["overlap"] > 0) == (hit >= 0)).all() and _own(touching) == _own(contacts), "one step further along the path they touch"
