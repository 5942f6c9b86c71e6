"""GPU: boxes moved through the device-resident world with collision, sliding and step-up (cvx_world_move, cvx_world_move_device).

The rule is integer from end to end, so every comparison is byte for byte: the random worlds of the CPU test against the dense model of
tests/movemodel.py through both entry points, every lanesPerBody giving the same bytes; the mill fixtures and the procedural scene world against the
host build of the rule (tests/move_rules.cpp over the blob the device reads back), before and after a sphere carve and a fill that move blocks to
the tails and rebuild columns; a repeating world; body counts around a wave; and a draw before and after, which the moves must not change."""
import numpy as np
import pytest
import torch

import movemodel
import ruleslib
import scenes
from cpuvox_amd import gpu
from test_gpu_world_edit import DIMS, _check_world, _context, _frames
from test_world_brush_cpu import _pick_world
from test_world_move_cpu import WORLDS, bodies_to_array, model_results, random_body, run_world, world_bodies

pytestmark = pytest.mark.gpu

U = gpu.MOVE_UNIT
LANES = (0, 1, 4, 16, 64)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("move_rules", tmp_path_factory.mktemp("move"), "-O2")


def _device_move(ctx, bodies, lanes):
    """cvx_world_move_device on the context's stream over torch buffers -> a MOVE_RESULT_DTYPE array"""
    d_bodies = torch.from_numpy(np.ascontiguousarray(bodies).view(np.int32).reshape(-1, 12).copy()).cuda()
    d_results = torch.full((len(bodies), 4), 0x55, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.world_move_device(len(bodies), d_bodies.data_ptr(), d_results.data_ptr(), lanes)
    ctx.synchronize()
    return d_results.cpu().numpy().reshape(-1).view(gpu.MOVE_RESULT_DTYPE).copy()


def _assert_all_routes(ctx, bodies, want, label):
    """the host-array call and the device call with every lanesPerBody give `want`, byte for byte"""
    got = ctx.world_move(bodies)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"{label}: host-array call: {len(bad)} of {len(bodies)} bodies differ; first {bodies[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"
    for lanes in LANES:
        got = _device_move(ctx, bodies, lanes)
        bad = np.flatnonzero(got != want)
        assert not len(bad), f"{label}: lanesPerBody {lanes}: {len(bad)} of {len(bodies)} bodies differ; first {bodies[bad[0]]}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---- the random worlds of the CPU test against the model -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse,seed", WORLDS)
def test_random_worlds_match_the_model_through_both_entry_points(dims, sparse, seed):
    """Records with 1 .. 3 runs, run-list columns, both colour layouts; the CPU test's bodies (starts outside and embedded, every flag combination,
    sizes up to the maximum); bounded and repeating (a world 16 columns wide cannot repeat)."""
    solid, _, ws = _pick_world(np.random.default_rng(seed), dims, sparse)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        for repeat in (False, True) if min(dims[0], dims[2]) >= 32 else (False,):
            ctx.set_world_repeat(repeat)
            bodies = world_bodies(seed, solid, repeat, 1500)
            want = model_results(solid, bodies, repeat)
            assert (want["flags"] & movemodel.RESTING).astype(bool).sum() > 100 and (want["flags"] & movemodel.STARTS_SOLID).astype(bool).sum() > 50
            _assert_all_routes(ctx, bodies_to_array(bodies), want, f"{dims} repeat {repeat}")
    finally:
        ctx.close()
        ws.close()


def test_a_full_wave_of_64_distinct_bodies_and_counts_around_it():
    """64 bodies that differ in size, delta, flags and stepUp share one wave at a thread per body; 1, 63, 64 and 65 bodies end inside a wave,
    at its end and one past it for every lanesPerBody."""
    solid, _, ws = _pick_world(np.random.default_rng(21), (32, 32, 32), False)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        bodies = world_bodies(21, solid, False, 65)
        assert len({tuple(b["size"]) + tuple(b["delta"]) for b in bodies[:64]}) == 64
        want = model_results(solid, bodies, False)
        for count in (1, 63, 64, 65):
            _assert_all_routes(ctx, bodies_to_array(bodies[:count]), want[:count], f"{count} bodies")
    finally:
        ctx.close()
        ws.close()


# ---- the fixture worlds against the host build of the rule, before and after edits ----------------------------------------------------------------------

def _surface_bodies(ctx, dims, n, seed):
    """n random bodies over a large world: half of them start where a first call dropped them (on the ground, against walls), with new deltas."""
    rng = np.random.default_rng(seed)
    bodies = bodies_to_array([random_body(rng, dims, big=0.01) for _ in range(n)])
    drop = bodies.copy()
    drop["delta"][:, 1] = -movemodel.MAX_DELTA
    landed = ctx.world_move(drop)
    settle = rng.random(n) < 0.5
    bodies["pos"][settle] = landed["pos"][settle]
    return bodies


@pytest.mark.parametrize("name", ["mill256", "mill512", "proc256"])
def test_fixture_worlds_match_the_host_rule_before_and_after_edits(rules, tmp_path, name):
    ws = scenes.load_world(name)
    dims = tuple(ws.dims)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        bodies = _surface_bodies(ctx, dims, 10000, 31)
        cx, cz = dims[0] // 2, dims[2] // 2
        edits = [None,
                 [{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_SPHERE, "a": (cx, dims[1] // 4, cz), "radius": dims[0] // 5}],
                 [{"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": (cx - 40, 0, cz - 9), "b": (cx + 40, dims[1] // 2, cz + 9), "argb": 0xFF112233}]]
        for k, strokes in enumerate(edits):
            if strokes:
                ctx.brush(strokes)
            blob, columns = ctx.read_level(0)
            for repeat in (False, True):
                ctx.set_world_repeat(repeat)
                want, _, _, _ = run_world(rules, tmp_path, blob, dims, columns, repeat, bodies)
                if k == 0 and not repeat:
                    flags = want["flags"]
                    assert (flags & movemodel.RESTING).astype(bool).sum() > 500 and (flags & 0x33).astype(bool).sum() > 300, "the bodies must meet the world"
                    assert not (flags & movemodel.INVALID).any()
                _assert_all_routes(ctx, bodies, want, f"{name} after {k} edits, repeat {repeat}")
            ctx.set_world_repeat(False)
    finally:
        ctx.close()


# ---- what the calls leave alone, and what they refuse ----------------------------------------------------------------------------------------------------

def test_moves_change_neither_the_world_nor_what_both_kernels_render():
    solid, _, ws = _pick_world(np.random.default_rng(41), DIMS, False)
    ctx = _context(ws)
    try:
        frames = _frames(ws)[:2]
        _check_world(ctx, ws, frames, "before the moves")
        before = [ctx.read_level(k)[0] for k in range(6)]
        bodies = world_bodies(41, solid, False, 2000)
        _assert_all_routes(ctx, bodies_to_array(bodies), model_results(solid, bodies, False), "between the draws")
        assert [ctx.read_level(k)[0] for k in range(6)] == before
        _check_world(ctx, ws, frames, "after the moves")
    finally:
        ctx.close()
        ws.close()


def test_bodies_outside_the_limits():
    """The host-array call refuses the whole call; the device call cannot look: the kernel answers such a body with its pos and CVX_MOVED_INVALID,
    and moves the others."""
    solid, _, ws = _pick_world(np.random.default_rng(42), (32, 32, 32), False)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        good = world_bodies(42, solid, False, 130)
        bad = {3: movemodel.body((5, 6, 7), (0, 1, 1)), 64: movemodel.body((5, 6, 7), (1, 1, 1), (0, 0, 256 * U + 1)), 65: movemodel.body((2**28 + 1, 0, 0), (9, 9, 9)),
               100: movemodel.body((1, 2, 3), (1, 1, 1), step_up=-1), 129: movemodel.body((-2**31, 2**31 - 1, 0), (2**31 - 1, 1, 1), (2**31 - 1, -2**31, 0), 2**31 - 1, -1)}
        mixed = [bad.get(i, b) for i, b in enumerate(good)]
        want = model_results(solid, mixed, False)
        assert sorted(np.flatnonzero(want["flags"] == movemodel.INVALID)) == sorted(bad)
        for lanes in LANES:
            got = _device_move(ctx, bodies_to_array(mixed), lanes)
            assert (got == want).all(), f"lanesPerBody {lanes}"
        with pytest.raises(gpu.CvxError, match="body 3"):
            ctx.world_move(bodies_to_array(mixed))
        for lanes in (-1, 2, 8, 32, 128):
            with pytest.raises(gpu.CvxError, match="lanesPerBody"):
                _device_move(ctx, bodies_to_array(good), lanes)
        with pytest.raises(gpu.CvxError):
            ctx.world_move([])
    finally:
        ctx.close()
        ws.close()
