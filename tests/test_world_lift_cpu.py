"""CPU (no GPU needed): the rules behind cvx_world_lift_pieces (cpuvox_amd/csrc/cvx_lift.h), compiled for the host through tests/lift_rules.cpp,
and the dense model of tests/liftmodel.py the GPU test compares the call with.  Integers and bytes throughout; the one comparison with a
tolerance is cvx_lifted_piece_mass against exact rationals.

- LiftNodeSums against brute-force sums for every interval of a 40-high column at several (x, z), and at extents 65535, where the piece's sums
  wrap, against Python integers modulo 2^64.
- LiftPlan on the capacity edges, LiftElement against numpy's ravel order (indices past 2^32 among them).
- cvx_lifted_piece_mass (the library's, and the rule through the stand-alone program) against fractions.Fraction on random pieces and on a
  single voxel.
- The same program under the address and undefined-behaviour sanitizers.
- The argument checks that need no device.
- The model on hand-made worlds.
- The Python wrappers and the documents (the header's mirrors: tests/test_abi_mirrors.py)."""
import os
import subprocess

import numpy as np
import pytest

import liftmodel
import piecesmodel
import ruleslib
from cpuvox_amd import gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD = 1 << 64


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("lift_rules", tmp_path_factory.mktemp("lift"))


def run(program, mode, tmp_path, words, in_dtype, out_dtype, env=None):
    src, dst = tmp_path / f"{mode}.in", tmp_path / f"{mode}.out"
    src.write_bytes(np.asarray(words, dtype=in_dtype).tobytes())
    subprocess.check_call([program, mode, str(src), str(dst)], env=env)
    return np.frombuffer(dst.read_bytes(), dtype=out_dtype)


# ---- LiftNodeSums ------------------------------------------------------------------------------------------------------------------------------------

def brute_sums(px, pz, lo, hi):
    """The nine sums of the voxels (px, y, pz), lo <= y < hi, voxel by voxel in Python integers."""
    ys = range(lo, hi)
    n, sy, syy = len(ys), sum(ys), sum(y * y for y in ys)
    return [n * px, sy, n * pz, n * px * px, syy, n * pz * pz, px * sy, sy * pz, n * pz * px]


def check_node_sums(program, tmp_path, env=None):
    nodes = [(px, pz, lo, hi) for px, pz in ((0, 0), (1, 0), (0, 1), (5, 9), (63, 127), (65534, 65533)) for lo in range(40) for hi in range(lo + 1, 41)]
    got = run(program, "sums", tmp_path, nodes, np.uint64, np.uint64, env).reshape(-1, 9)
    want = [brute_sums(*node) for node in nodes]
    assert len(got) == len(nodes) + 1 == 6 * 820 + 1
    bad = [(node, g.tolist(), w) for node, g, w in zip(nodes, got, want) if g.tolist() != w]
    assert not bad, bad[:3]
    assert got[-1].tolist() == [sum(w[k] for w in want) % MOD for k in range(9)]


def check_sums_wrap(program, tmp_path, env=None):
    """Extents of 65535: 60 random nodes voxel by voxel, then 70 000 full columns at the far corner of the box, whose p_x^2 sum alone passes 2^64."""
    rng = np.random.default_rng(5)
    nodes = []
    for _ in range(60):
        lo = int(rng.integers(0, 65535))
        nodes.append((int(rng.integers(0, 65535)), int(rng.integers(0, 65535)), lo, int(rng.integers(lo + 1, 65536))))
    nodes += [(0, 0, 0, 65535), (65534, 65534, 65534, 65535), (65534, 0, 0, 1)]
    far = (65534, 65534, 0, 65535)
    want = [brute_sums(*node) for node in nodes]
    far_sums = brute_sums(*far)
    got = run(program, "sums", tmp_path, nodes + [far] * 70000, np.uint64, np.uint64, env).reshape(-1, 9)
    assert [g.tolist() for g in got[:len(nodes)]] == want
    assert got[len(nodes)].tolist() == far_sums == got[-2].tolist()
    exact = [sum(w[k] for w in want) + 70000 * far_sums[k] for k in range(9)]
    assert exact[3] >= MOD and exact[5] >= MOD and exact[8] >= MOD and exact[4] < MOD, "the squares of x and z and their product wrap, the rest does not"
    assert got[-1].tolist() == [v % MOD for v in exact]


def test_node_sums_equal_brute_force_for_every_interval_of_a_column(rules, tmp_path):
    check_node_sums(rules, tmp_path)


def test_node_sums_at_extents_of_65535_wrap_modulo_2_to_the_64(rules, tmp_path):
    check_sums_wrap(rules, tmp_path)


# ---- LiftPlan, LiftElement ---------------------------------------------------------------------------------------------------------------------------

def plan_model(capacity, boxes):
    """The header's prefix rule: (offsets, storedPieces, storedVoxels)."""
    offsets, used, open_ = [], 0, True
    for mn, mx in boxes:
        v = (mx[0] - mn[0]) * (mx[1] - mn[1]) * (mx[2] - mn[2])
        open_ = open_ and used + v <= capacity
        offsets.append(used if open_ else -1)
        used += v if open_ else 0
    return offsets, sum(o >= 0 for o in offsets), used


def plan_cases():
    boxes = [((3, 4, 5), (5, 7, 6)), ((0, 0, 0), (1, 1, 1)), ((-4, 10, 2), (6, 12, 5)), ((7, 7, 7), (8, 9, 8)), ((1, 2, 3), (4, 4, 9))]  # volumes 6 1 60 2 36
    volumes = [6, 1, 60, 2, 36]
    cases = [(0, boxes), (10 ** 18, boxes), ((1 << 63) - 1, boxes), (0, []), (50, [])]
    for k in range(1, 6):  # the sum of the first k volumes, and one less
        cases += [(sum(volumes[:k]), boxes), (sum(volumes[:k]) - 1, boxes)]
    cases.append((5, boxes))                   # the first piece does not fit: nothing is stored, although the second would
    cases.append((66, boxes[2:] + boxes[:2]))  # 60 fits, 2 fits, 36 does not; the 6 and the 1 behind it are NOT stored (a prefix)
    big = [((0, 0, 0), (65535, 65535, 65535)), ((0, 0, 0), (65535, 65535, 65535)), ((0, 0, 0), (2, 2, 2))]
    cases += [(65535 ** 3, big), (2 * 65535 ** 3 + 7, big), ((1 << 63) - 1, big * 8)]
    return cases


def check_plan(program, tmp_path, env=None):
    cases = plan_cases()
    words = []
    for capacity, boxes in cases:
        words += [capacity, len(boxes)]
        for mn, mx in boxes:
            words += [*mn, *mx]
    got = run(program, "plan", tmp_path, words, np.int64, np.int64, env).tolist()
    at = 0
    for capacity, boxes in cases:
        offsets, pieces, voxels = plan_model(capacity, boxes)
        assert got[at:at + len(boxes) + 2] == offsets + [pieces, voxels], (capacity, boxes)
        at += len(boxes) + 2
    assert at == len(got)
    assert plan_model(66, cases[16][1])[0] == [0, 60, -1, -1, -1] and plan_model(5, cases[15][1])[1:] == (0, 0)


def check_element(program, tmp_path, env=None):
    rng = np.random.default_rng(11)
    cases, want = [], []
    for shape in [(1, 1, 1), (3, 5, 7), (7, 1, 2), (1, 9, 1), (64, 128, 64), (3000, 1000, 2000), (65535, 65535, 65535)]:  # (X, Y, Z)
        sx, sy, sz = shape
        points = [(0, 0, 0), (sx - 1, sy - 1, sz - 1)] + [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(50)]
        for px, py, pz in points:
            cases.append((px, py, pz, sy, sz))
            want.append((px * sz + pz) * sy + py)
            if sx * sy * sz < 1 << 62:
                assert want[-1] == int(np.ravel_multi_index((px, pz, py), (sx, sz, sy))), "the layout is numpy's ravel order of an (X, Z, Y) array"
    got = run(program, "element", tmp_path, cases, np.int64, np.int64, env).tolist()
    assert got == want and max(want) > 1 << 47
    small = np.arange(3 * 7 * 5).reshape(3, 7, 5)  # (X, Z, Y)
    words = [(x, y, z, 5, 7) for x in range(3) for z in range(7) for y in range(5)]
    assert run(program, "element", tmp_path, words, np.int64, np.int64, env).tolist() == small.ravel().tolist()


def test_the_plan_stores_the_longest_prefix_that_fits(rules, tmp_path):
    check_plan(rules, tmp_path)


def test_the_element_index_is_numpys_ravel_order(rules, tmp_path):
    check_element(rules, tmp_path)


# ---- cvx_lifted_piece_mass ---------------------------------------------------------------------------------------------------------------------------

def random_pieces():
    """LIFTED_PIECE_DTYPE elements of random voxel sets (connectedness does not matter to the sums): blobs, plates, rods, a lopsided dumbbell."""
    rng = np.random.default_rng(29)
    out = []
    for k in range(40):
        shape = [(12, 30, 9), (40, 2, 40), (1, 100, 1), (25, 25, 25)][k % 4]
        cells = rng.random(shape) < (0.05, 0.5, 0.9, 0.3)[k % 4]
        if k % 8 == 7:  # nearly all of the mass in one corner, one voxel far away
            cells[:] = False
            cells[:3, :3, :3] = True
            cells[-1, -1, -1] = True
        p = np.argwhere(cells)
        if len(p) == 0:
            continue
        mn = p.min(axis=0)
        piece = np.zeros((), dtype=liftmodel.LIFTED_PIECE_DTYPE)
        piece["piece"]["min"] = mn + rng.integers(0, 1000, 3)
        piece["piece"]["max"] = piece["piece"]["min"] + (p.max(axis=0) + 1 - mn)
        piece["piece"]["voxels"] = len(p)
        piece["sum"], piece["moment"] = liftmodel.sums_of(p - mn)
        out.append(piece)
    return np.array(out, dtype=liftmodel.LIFTED_PIECE_DTYPE)


def single_voxel(at=(17, 3, 250)):
    piece = np.zeros((), dtype=liftmodel.LIFTED_PIECE_DTYPE)
    piece["piece"]["min"], piece["piece"]["max"], piece["piece"]["seed"], piece["piece"]["voxels"] = at, [v + 1 for v in at], at, 1
    return piece


def check_mass(results, pieces):
    """results: (n, 9) doubles, centre then inertia.  At most 1e-12 of the largest entry off the exact rationals: a few dozen roundings of
    1.1e-16 each, and the cancellation in m - s^2 / n is bounded by the pieces' shapes (the lopsided one is the worst here)."""
    assert results.shape == (len(pieces), 9)
    worst = 0.0
    for got, piece in zip(results, pieces):
        centre, inertia = liftmodel.mass(piece)
        for exact, values in ((centre, got[:3]), (inertia, got[3:])):
            scale = max(abs(v) for v in exact)
            errors = [abs(float(abs(v - e_) / scale)) for v, e_ in zip((liftmodel.Fraction(float(g)) for g in values), exact)]
            worst = max(worst, *errors)
            assert max(errors) <= 1e-12, (piece, values, [float(e_) for e_ in exact])
    return worst


def test_mass_properties_against_exact_rationals(rules, tmp_path):
    pieces = random_pieces()
    assert len(pieces) >= 35
    through_rules = run(rules, "mass", tmp_path, pieces, liftmodel.LIFTED_PIECE_DTYPE, np.float64).reshape(-1, 9)
    through_library = np.array([np.concatenate(gpu.lifted_piece_mass(p)) for p in pieces])
    assert through_rules.tobytes() == through_library.tobytes(), "cvx_lifted_piece_mass is the rule"
    check_mass(through_rules, pieces)


def test_a_single_voxel_has_its_centre_in_the_middle_and_a_third_on_the_diagonal():
    centre, inertia = gpu.lifted_piece_mass(single_voxel())
    assert centre.tolist() == [17.5, 3.5, 250.5]
    assert inertia.tolist() == [1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0, 0.0, 0.0, 0.0]
    assert liftmodel.mass(single_voxel()) == ([liftmodel.Fraction(35, 2), liftmodel.Fraction(7, 2), liftmodel.Fraction(501, 2)],
                                              [liftmodel.Fraction(1, 3)] * 3 + [0, 0, 0])
    two = single_voxel((0, 0, 0))  # two voxels side by side in x: the parallel-axis term 2 * (1/2)^2 on the two axes across
    two["piece"]["max"], two["piece"]["voxels"], two["sum"], two["moment"] = (2, 1, 1), 2, (1, 0, 0), (1, 0, 0, 0, 0, 0)
    centre, inertia = gpu.lifted_piece_mass(two)
    assert centre.tolist() == [1.0, 0.5, 0.5] and inertia.tolist() == [2.0 / 3.0, 0.5 + 2.0 / 3.0, 0.5 + 2.0 / 3.0, 0.0, 0.0, 0.0]
    empty = single_voxel()
    empty["piece"]["voxels"] = 0
    with pytest.raises(ValueError):
        gpu.lifted_piece_mass(empty)


# ---- the sanitizers ----------------------------------------------------------------------------------------------------------------------------------

def test_the_rules_are_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python, nothing of the library is linked) built with
    -fsanitize=address,undefined: every check above runs to the end with the same results."""
    program = ruleslib.build("lift_rules", tmp_path, "-g", "-DLIFT_RULES_NO_LIBRARY", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", link_library=False)
    check_node_sums(program, tmp_path)
    check_sums_wrap(program, tmp_path)
    check_plan(program, tmp_path)
    check_element(program, tmp_path)
    pieces = random_pieces()
    check_mass(run(program, "mass", tmp_path, pieces, liftmodel.LIFTED_PIECE_DTYPE, np.float64).reshape(-1, 9), pieces)


# ---- the argument checks -----------------------------------------------------------------------------------------------------------------------------

def test_the_rejections_that_need_no_device(rules):
    lines = [line.split("|", 1) for line in subprocess.check_output([rules, "args"], text=True).splitlines()]
    got = [(int(code), message) for code, message in lines]
    want = [
        (-1, ""), (-1, ""), (-1, "the box is NULL"), (-1, "the box [8, 8) on axis 1 is empty"), (-1, "unknown anchors bits 0x8"),
        (-1, "bad op 2"), (-1, "bad op -1"), (-1, "voxelCapacity -1 is negative"), (-1, "voxelCapacity 4 with no pool"), (-1, "voxelCapacity 1 with no pool"),
        (-1, "levelCount 6 outside 0 .. 5"), (-1, "pieceCapacity -1 with a list"), (-1, "pieceCapacity 2 with no list"),
        (-3, "world LOD 0 has not been uploaded"),
        (1, "untouched"),
        (-1, ""), (-1, ""), (-1, ""), (0, ""),
    ]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w] or (len(got), len(want))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------

def interlocked(dims=(32, 32, 32)):
    """A U-frame lying in the XY plane and a bar through its opening, one voxel clear of it on every side: two pieces, the bar's box inside the
    frame's.  -> (solid, colour)"""
    solid = np.zeros(dims, dtype=bool)
    solid[:, 0, :] = True
    solid[8:20, 10:12, 14:17] = True    # the U's bottom ...
    solid[8:10, 12:20, 14:17] = True    # ... and its two arms
    solid[18:20, 12:20, 14:17] = True
    solid[11:17, 13:15, 4:28] = True    # the bar along z through the opening (x 10 .. 17, y 12 .. 19), one voxel clear of the arms and the bottom
    x, y, z = np.nonzero(solid)
    colour = np.zeros(dims, dtype=np.uint32)
    colour[x, y, z] = 0xFF000000 | (x << 16) | (y << 8) | z
    return solid, colour


def test_the_model_on_two_interlocked_pieces():
    solid, colour = interlocked()
    whole = ((0, 0, 0), solid.shape)
    want = liftmodel.lift(solid, colour, *whole, piecesmodel.GROUND, 8, 10 ** 9)
    assert want.summary["floatingPieces"] == 2 == want.summary["storedPieces"]
    frame, bar = want.pieces
    assert frame["piece"]["min"].tolist() == [8, 10, 14] and frame["piece"]["max"].tolist() == [20, 20, 17] and int(frame["offset"]) == 0
    assert bar["piece"]["min"].tolist() == [11, 13, 4] and bar["piece"]["max"].tolist() == [17, 15, 28] and int(bar["offset"]) == 12 * 10 * 3
    assert want.summary["storedVoxels"] == want.summary["neededVoxels"] == 360 + 6 * 2 * 24 == len(want.argb) == len(want.solid)
    frame_argb, frame_solid = want.models[0]
    assert frame_solid.shape == (12, 3, 10) and int(frame_solid.sum()) == int(frame["piece"]["voxels"]) == 12 * 2 * 3 + 2 * 2 * 8 * 3
    assert not frame_solid[3:9, :, 3:5].any(), "the bar's voxels inside the frame's box are not the frame's"
    assert frame_argb[0, 0, 0] == 0xFF000000 | (8 << 16) | (10 << 8) | 14 and (frame_argb != 0).sum() == frame_solid.sum()
    assert int(bar["sum"][2]) == 6 * 2 * sum(range(24)) and int(bar["moment"][2]) == 12 * sum(k * k for k in range(24))
    # capacity one short of both: the frame alone; REMOVE leaves the bar
    less = liftmodel.lift(solid, colour, *whole, piecesmodel.GROUND, 8, 360 + 287)
    assert less.summary["storedPieces"] == 1 and less.pieces["offset"].tolist() == [0, -1] and less.summary["neededVoxels"] == 648
    assert less.pieces["sum"].tolist() == want.pieces["sum"].tolist(), "the sums do not depend on what is stored"
    after, _ = less.removed
    assert after[11, 13, 4] and not after[8, 10, 14] and int(after.sum()) == int(solid.sum()) - int(frame["piece"]["voxels"])
    # the list capacity bounds what is stored too
    one = liftmodel.lift(solid, colour, *whole, piecesmodel.GROUND, 1, 10 ** 9)
    assert len(one.pieces) == 1 and one.summary["storedPieces"] == 1 and one.summary["floatingPieces"] == 2 and one.summary["neededVoxels"] == 648


# ---- wrappers and documents ----------------------------------------------------------------------------------------------------------------------------------------

def test_python_wrappers():
    assert hasattr(gpu.Context, "world_lift_pieces") and hasattr(gpu.Context, "world_lift_pieces_device") and callable(gpu.lifted_model)
    pieces = np.zeros(2, dtype=gpu.LIFTED_PIECE_DTYPE)
    pieces["piece"]["max"] = [(2, 3, 4), (1, 1, 1)]
    pieces["offset"] = [5, -1]
    pool = np.arange(40, dtype=np.uint32)
    size, argb, solid = gpu.lifted_model(pieces, 0, pool, None)
    assert size == (2, 3, 4) and solid is None and argb.shape == (2, 4, 3) and argb[0, 0, 0] == 5 and argb[1, 3, 2] == 28 and argb.base is not None
    assert gpu.lifted_model(pieces, 0, 4096, 8192) == ((2, 3, 4), 4096 + 20, 8192 + 5)
    with pytest.raises(ValueError, match="not stored"):
        gpu.lifted_model(pieces, 1, pool, None)


def test_the_documents_name_the_call():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"all {len(gpu.EXPORTS)} exports" in readme
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("tools", "README.md"), os.path.join("profiles", "lift.md")):
        assert "cvx_world_lift_pieces" in open(os.path.join(ROOT, name)).read(), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "cvx_lifted_piece_mass" in integration and "cvx_world_place_models_device" in integration
