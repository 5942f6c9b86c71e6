"""CPU (no GPU needed): the rule behind cvx_world_surface (cpuvox_amd/csrc/cvx_surface.h), compiled for the host through tests/surface_rules.cpp
(which drives it as the device does: count, prefix sum, write), against the independent dense model of tests/surfacemodel.py.

- Column mode: 2000 random small worlds (seed 4099) of up to 4 x 4 random columns (records with 1..3 runs and listed columns, both colour
  layouts, foreign encodings with split runs and shared colours, empty columns; in half of the cases the colours are folded onto three values so
  that neighbouring voxels often share one) with random boxes (partly outside the world), random solidOutside 0 .. 63 and both flag values: the
  summary and every quad must equal the model's bytes.  What the cases have to cover is asserted from the model first.
- World mode: the three _pick_world worlds and the two noise worlds uploaded into a host-only context.
- Properties, of the model and of the rule: unitFaces is the sum of the lengths, the surface of a whole world with air outside is closed, and
  eight sub-boxes give the unit faces of one call.
- cvx_surface_triangles: winding, areas, planes, indices and the colour round trip through the stamp rule's packing.
- The calls without a context / world and every INVALID_ARGUMENT case (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import piecesmodel
import ruleslib
import surfacemodel
from cpuvox_amd import gpu
from test_world_brush_cpu import _pick_world, _random_column
from test_world_cavities_cpu import NOISE_DIMS, noise_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = surfacemodel.IGNORE_COLOUR


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("surface_rules", tmp_path_factory.mktemp("surface"))


def random_call(rng, dims):
    """(box_min, box_max, solid_outside, flags): a random box partly outside the world (the whole world when nothing of it is inside)."""
    box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
    box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
    if piecesmodel.clip_box(dims, box_min, box_max) is None:
        box_min, box_max = [0, 0, 0], list(dims)
    return box_min, box_max, int(rng.integers(0, 64)), int(rng.integers(0, 2))


def parse(raw, count=None):
    """The bytes surface_rules writes -> [(summary dict, quads array)]."""
    out, at = [], 0
    while at < len(raw):
        s = np.frombuffer(raw[at:at + 64], dtype=gpu.SURFACE_SUMMARY_DTYPE)[0]
        n = int(s["quads"])
        quads = np.frombuffer(raw[at + 64:at + 64 + 24 * n], dtype=gpu.SURFACE_QUAD_DTYPE)
        out.append(({"quads": n, "unitFaces": int(s["unitFaces"]), "quadsPerFace": [int(v) for v in s["quadsPerFace"]]}, quads))
        at += 64 + 24 * n
    assert at == len(raw) and (count is None or len(out) == count)
    return out


# ---- column mode -------------------------------------------------------------------------------------------------------------------------------

def _run_columns(rules, tmp_path, cases):
    words = []
    for dim_y, gx, gz, stride, columns, box_min, box_max, solid_outside, flags in cases:
        words += ruleslib.world_words(dim_y, gx, gz, stride, columns) + list(box_min) + list(box_max) + [solid_outside, flags]
    return parse(ruleslib.run_cases(rules, "columns", tmp_path, words, dtype=np.uint8).tobytes(), len(cases))


def _fold(c):
    """Three colour words instead of 2^32, so that voxels above each other often share one."""
    return np.uint32(0xFF000010) + (np.asarray(c, dtype=np.uint32) % np.uint32(3)).astype(np.uint32)


def test_rule_matches_the_dense_model_on_random_small_worlds(rules, tmp_path):
    rng = np.random.default_rng(4099)
    cases, models = [], []
    split = listed_like = empty = 0
    long_quads = by_colour = by_box = no_quad = 0
    boundary = np.zeros((6, 2), dtype=np.int64)  # per world face: quads emitted on it, faces suppressed on it
    for _ in range(2000):
        dim_y = int(rng.choice([8, 16, 64, 256]))
        gx, gz = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        stride = int(rng.choice([1, 32]))
        fold = rng.random() < 0.5
        solid = np.zeros((gx, dim_y, gz), dtype=bool)
        colour = np.zeros((gx, dim_y, gz), dtype=np.uint32)
        columns = []
        for k in range(gx * gz):
            runs, colours, _, dense = _random_column(rng, dim_y)
            if fold:
                colours, dense = [int(v) for v in _fold(colours)] if len(colours) else [], _fold(dense)
            x, z = k // gz, k % gz
            colour[x, :, z] = dense
            top = dim_y
            previous_solid = False
            for ci, n in runs:
                if ci >= 0:
                    solid[x, top - n:top, z] = True
                    split += previous_solid
                previous_solid = ci >= 0
                top -= n
            columns.append((32 + k * 20000 + int(rng.integers(0, 100)), runs, colours))
            listed_like += sum(1 for ci, _ in runs if ci >= 0) > 3
            empty += not runs
        colour[~solid] = 0
        dims = (gx, dim_y, gz)
        box_min, box_max, solid_outside, flags = random_call(rng, dims)
        if rng.random() < 0.3:
            box_min, box_max = [0, 0, 0], list(dims)
        cases.append((dim_y, gx, gz, stride, columns, box_min, box_max, solid_outside, flags))
        quads, summary = surfacemodel.surface(solid, colour, box_min, box_max, solid_outside, flags)
        models.append((summary, quads))
        # what the cases cover, from the model
        lo, hi = piecesmodel.clip_box(dims, box_min, box_max)
        side = np.isin(quads["face"], (0, 1, 4, 5))
        long_quads += int((quads["length"] >= 3).sum())
        per_column = np.zeros((gx, gz), dtype=np.int64)
        np.add.at(per_column, (quads["voxel"][:, 0], quads["voxel"][:, 2]), 1)
        no_quad += int((per_column[lo[0]:hi[0], lo[2]:hi[2]] == 0).sum())
        exposed = surfacemodel.exposed(solid, solid_outside)
        for q in quads[side]:
            x, y, z = (int(v) for v in q["voxel"])
            f = int(q["face"])
            if y > lo[1] and exposed[f][x, y - 1, z]:  # the voxel below is exposed too and inside the y range: only its colour ended the quad
                by_colour += not flags and colour[x, y - 1, z] != q["argb"]
            if y == lo[1] and y > 0 and exposed[f][x, y - 1, z] and (flags or colour[x, y - 1, z] == q["argb"]):
                by_box += 1  # the quad would go on below the box
        for f in range(6):
            a, up = f // 2, f % 2
            at = dims[a] - 1 if up else 0
            if not (lo[a] <= at < hi[a]):
                continue
            on_face = quads[(quads["face"] == f) & ((quads["voxel"][:, a] + (quads["length"] - 1 if a == 1 and up else 0)) == at)]
            plane = [slice(lo[0], hi[0]), slice(lo[1], hi[1]), slice(lo[2], hi[2])]
            plane[a] = at
            boundary[f, 0] += len(on_face)
            boundary[f, 1] += int(solid[tuple(plane)].sum()) if (solid_outside >> f) & 1 else 0
    results = _run_columns(rules, tmp_path, cases)
    bad = [i for i, (got, want) in enumerate(zip(results, models)) if got[0] != want[0] or got[1].tobytes() != want[1].tobytes()]
    if bad:
        i = bad[0]
        raise AssertionError(f"{len(bad)} of {len(cases)} cases differ; first: case {i} {cases[i]}\n got {results[i][0]}\n{results[i][1]}\nwant {models[i][0]}\n{models[i][1]}")
    assert split > 100 and listed_like > 300 and empty > 100, (split, listed_like, empty)
    assert long_quads > 1000 and by_colour > 1000 and by_box > 100 and no_quad > 100, (long_quads, by_colour, by_box, no_quad)
    assert (boundary > 20).all(), boundary.tolist()


# ---- world mode ---------------------------------------------------------------------------------------------------------------------------------

def run_world(rules, tmp_path, ws, box_min, box_max, solid_outside, flags):
    """tests/surface_rules.cpp `world` on LOD 0 of ws -> (summary dict, quads array, host milliseconds of the walk)."""
    info = ws.info(0)
    blob, out = tmp_path / "world.bin", tmp_path / "quads.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                    *[str(int(v)) for v in box_min], *[str(int(v)) for v in box_max], str(solid_outside), str(flags), str(out)], text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) ms ([0-9.]+)", text)
    assert m, text
    (summary, quads), = parse(out.read_bytes(), 1)
    return summary, quads, float(m.group(3))


def world_boxes(dims):
    """Named (box_min, box_max, solid_outside, flags) over a world of `dims` (the GPU test uses them too)."""
    dx, dy, dz = dims
    return {
        "whole world, ground below": ((0, 0, 0), dims, 0x04, 0),
        "whole world, collision mesh": ((0, 0, 0), dims, 0x04, IGNORE),
        "whole world, air outside": ((0, 0, 0), dims, 0, 0),
        "whole world, solid outside": ((0, 0, 0), dims, 0x3F, IGNORE),
        "inner box": ((3, 2, 5), (dx - 4, dy - 3, dz - 2), 0x04, 0),
        "inner box, collision mesh": ((3, 2, 5), (dx - 4, dy - 3, dz - 2), 0x3B, IGNORE),
        "upper half": ((0, dy // 4, 0), (dx, dy, dz), 0x04, 0),
        "partly outside the world": ((-5, -3, dz // 2), (dx // 2, dy + 9, dz + 4), 0x15, 0),
        "one column": ((3, 0, 1), (4, dy, 2), 0x04, 0),
        "one voxel": ((3, dy // 4 - 2, 1), (4, dy // 4 - 1, 2), 0x04, 0),
    }


def _check_calls(rules, tmp_path, solid, colour, ws, calls):
    for name, (box_min, box_max, solid_outside, flags) in calls.items():
        want, want_summary = surfacemodel.surface(solid, colour, box_min, box_max, solid_outside, flags)
        summary, quads, _ = run_world(rules, tmp_path, ws, box_min, box_max, solid_outside, flags)
        assert summary == want_summary, name
        assert quads.tobytes() == want.tobytes(), name


@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((32, 128, 32), True, 3)])
def test_terrain_worlds_equal_the_model(rules, tmp_path, dims, sparse, seed):
    solid, colour, ws = _pick_world(np.random.default_rng(seed), dims, sparse)
    try:
        _check_calls(rules, tmp_path, solid, colour, ws, world_boxes(dims))
    finally:
        ws.close()


@pytest.mark.parametrize("dims", NOISE_DIMS)
def test_noise_worlds_with_random_boxes(rules, tmp_path, dims):
    solid, colour, ws = noise_world(dims)
    try:
        calls = dict(world_boxes(dims))
        rng = np.random.default_rng(dims[0] + 7)
        for k in range(12):
            calls[f"random call {k}"] = random_call(rng, dims)
        _check_calls(rules, tmp_path, solid, colour, ws, calls)
    finally:
        ws.close()


# ---- properties ---------------------------------------------------------------------------------------------------------------------------------

def _rows(faces):
    return sorted(map(tuple, faces.tolist()))


@pytest.mark.parametrize("which", ["model", "rule"])
def test_closed_surface_and_tiling_sub_boxes(rules, tmp_path, which):
    dims = NOISE_DIMS[1]
    solid, colour, ws = noise_world(dims)
    try:
        def call(box_min, box_max, solid_outside, flags):
            if which == "model":
                quads, summary = surfacemodel.surface(solid, colour, box_min, box_max, solid_outside, flags)
            else:
                summary, quads, _ = run_world(rules, tmp_path, ws, box_min, box_max, solid_outside, flags)
            assert summary["unitFaces"] == int(quads["length"].sum()) and summary["quads"] == len(quads) == sum(summary["quadsPerFace"])
            return quads
        for flags in (0, IGNORE):
            whole = call((0, 0, 0), dims, 0, flags)
            faces = surfacemodel.unit_faces(whole)
            assert len(faces) > 10000 and surfacemodel.open_edges(faces) == 0, "the surface of a whole world in air is not closed"
            # with the ground solid the bottom faces are missing and their outer edges are open
            grounded = surfacemodel.unit_faces(call((0, 0, 0), dims, 0x04, flags))
            assert surfacemodel.open_edges(grounded) > 0
            # eight sub-boxes (cut off-centre): the same unit faces; more quads only where the y cut splits one
            cx, cy, cz = 5, 23, 13
            parts = [call((x0, y0, z0), (x1, y1, z1), 0, flags)
                     for x0, x1 in ((0, cx), (cx, dims[0])) for y0, y1 in ((0, cy), (cy, dims[1])) for z0, z1 in ((0, cz), (cz, dims[2]))]
            joined = np.concatenate(parts)
            assert _rows(surfacemodel.unit_faces(joined)) == _rows(faces)
            side = np.isin(whole["face"], (0, 1, 4, 5))
            crossing = int((side & (whole["voxel"][:, 1] < cy) & (whole["voxel"][:, 1] + whole["length"] > cy)).sum())
            assert len(joined) == len(whole) + crossing and (crossing > 0 or not flags)
    finally:
        ws.close()


# ---- cvx_surface_triangles ----------------------------------------------------------------------------------------------------------------------

def test_triangles_are_wound_outward_on_the_face_plane(rules):
    quads = np.zeros(12, dtype=gpu.SURFACE_QUAD_DTYPE)
    for f in range(6):
        quads[f] = ((3, 5, 7), f, 1, 0xFF112233)
        quads[6 + f] = ((10 + f, 2, 4), f, 1 if f in (2, 3) else 9, 0x80FFFE00 + f)
    vertices, indices = gpu.surface_triangles(quads)
    assert vertices.shape == (48,) and indices.shape == (72,)
    assert indices.reshape(12, 6).tolist() == [[4 * k + o for o in (0, 1, 2, 0, 2, 3)] for k in range(12)]
    assert (vertices["uv"] == 0).all() and (vertices["material"] == -1).all()
    for k, q in enumerate(quads):
        f, length = int(q["face"]), int(q["length"])
        axis, up = f // 2, f % 2
        p = vertices["position"][4 * k:4 * k + 4].astype(np.float64)
        plane = q["voxel"][axis] + (length if axis == 1 and up else up)
        assert (p[:, axis] == plane).all(), (k, p)
        lo = q["voxel"].astype(np.float64)
        hi = lo + np.array([1, length, 1])
        others = [a for a in range(3) if a != axis]
        assert sorted(map(tuple, p[:, others].tolist())) == sorted((u, v) for u in (lo[others[0]], hi[others[0]]) for v in (lo[others[1]], hi[others[1]]))
        outward = np.zeros(3)
        outward[axis] = 1 if up else -1
        area = 0.0
        for a, b, c in ((0, 1, 2), (0, 2, 3)):
            n = np.cross(p[b] - p[a], p[c] - p[a])
            assert np.dot(n, outward) > 0 and not n[others].any(), (k, n)
            area += np.linalg.norm(n) / 2
        assert area == length
        r, g, b = (int(q["argb"]) >> 8) & 0xFF, (int(q["argb"]) >> 16) & 0xFF, int(q["argb"]) >> 24
        assert vertices["rgba"][4 * k:4 * k + 4].tolist() == [[r, g, b, 255]] * 4
    # the colour round trip: the stamp rule's packing of that vertex colour gives back the word (its alpha byte is the stamp's 0xFF)
    words = [0xFF112233, 0x00000000, 0xFFFFFFFF, 0x80FFFE00, 0x12345678, 0xFF0180FE]
    out = [int(v) for v in subprocess.check_output([rules, "colours", *[str(w) for w in words]], text=True).split()]
    assert out == [(w & 0xFFFFFF00) | 0xFF for w in words]
    empty_v, empty_i = gpu.surface_triangles(np.zeros(0, dtype=gpu.SURFACE_QUAD_DTYPE))
    assert len(empty_v) == 0 and len(empty_i) == 0


# ---- layouts and entry points ------------------------------------------------------------------------------------------------------------------

def test_surface_fails_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    ms = C.c_float()
    for entry in (L.cvx_world_surface, L.cvx_world_surface_device):
        assert entry(None, lo, hi, gpu.SURFACE_OUTSIDE_DEFAULT, 0, None, 0, None, C.byref(ms)) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    # a context without a device (tests/surface_rules.cpp): every bad argument of both calls, then CVX_ERR_NOT_READY without a world, a box
    # outside an uploaded world, and cvx_surface_triangles' own checks
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 16 + [-3, -3] + [-1, -1] + [-1] * 5 + [0], codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_surface(h, lo, hi, gpu.SURFACE_OUTSIDE_DEFAULT, 0, None, 0, None, C.byref(ms)) == -3
        finally:
            L.cvx_destroy(h)
