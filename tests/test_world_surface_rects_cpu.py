"""CPU (no GPU needed): the rule behind cvx_world_surface_rects (cpuvox_amd/csrc/cvx_surface_rects.h), compiled for the host through
tests/surface_rects_rules.cpp (which drives it as the device does: strips, the first pass, the row pass, prefix sum, write), against the
independent dense model of tests/surfacerectsmodel.py.

- Random worlds of 16 x 16 x 8 voxels at five densities with two or three colours, both flag values, several solidOutside masks and boxes that cut
  the world on every side: the summary and every rectangle must equal the model's bytes; without the model, the rectangles' unit faces are the
  strips' unit faces, each once, and no two rectangles share a whole edge.
- The slab (130 x 3 x 70 voxels of one colour, 18 600 strips, 6 rectangles), a solid block coloured as a checkerboard (nothing merges with
  colours, everything without), an L-shaped floor, a box cut in two.
- cvx_surface_rect_triangles: equal to cvx_surface_triangles on single strips, wound outward on the face plane, areas that sum to unitFaces.
- The calls without a context / world and every INVALID_ARGUMENT case (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ruleslib
import surfacemodel
import surfacerectsmodel as model
from cpuvox_amd import gpu, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = surfacemodel.IGNORE_COLOUR
SLAB_DIMS = (256, 16, 128)
SLAB = ((10, 5, 3), (140, 8, 73))  # solid x 10..139, y 5..7, z 3..72


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("surface_rects_rules", tmp_path_factory.mktemp("surface_rects"))


def built_world(dims, solid, colour):
    x, y, z = np.nonzero(solid)
    return host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), colour[x, y, z], threads=2)


def summary_dict(s):
    return {"rects": int(s["rects"]), "strips": int(s["strips"]), "unitFaces": int(s["unitFaces"]), "rectsPerFace": [int(v) for v in s["rectsPerFace"]]}


def run_world(rules, tmp_path, ws, box_min, box_max, solid_outside, flags):
    """tests/surface_rects_rules.cpp `world` on LOD 0 of ws -> (summary dict, rectangles)."""
    info = ws.info(0)
    blob, out = tmp_path / "world.bin", tmp_path / "rects.bin"
    if not blob.exists():
        blob.write_bytes(ws.storage(0).tobytes())
    subprocess.check_call([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                           *[str(int(v)) for v in box_min], *[str(int(v)) for v in box_max], str(solid_outside), str(flags), str(out)])
    raw = out.read_bytes()
    summary = summary_dict(np.frombuffer(raw[:72], dtype=gpu.SURFACE_RECTS_SUMMARY_DTYPE)[0])
    rects = np.frombuffer(raw[72:], dtype=gpu.SURFACE_RECT_DTYPE)
    assert len(rects) == summary["rects"]
    return summary, rects


def rows(faces):
    """The (x, y, z, face) rows sorted, as bytes: equal bytes are equal multisets."""
    faces = np.ascontiguousarray(faces, dtype=np.int64)
    return faces[np.lexsort(faces.T[::-1])].tobytes()


def check_properties(rects, summary, strips, flags, box, label=""):
    """What follows from the rule, checked without the model of the merge: `strips` are cvx_world_surface's quads for the same call."""
    faces = model.unit_faces(rects)
    assert rows(faces) == rows(surfacemodel.unit_faces(strips)), f"{label}: the rectangles do not cover the strips' faces"
    assert len(np.unique(faces, axis=0)) == len(faces), f"{label}: a face is covered twice"
    assert model.whole_edge_pairs(rects, bool(flags & IGNORE)) == 0, f"{label}: two rectangles share a whole edge"
    assert summary["rects"] == len(rects) == sum(summary["rectsPerFace"]) and summary["strips"] == len(strips), label
    assert summary["unitFaces"] == int(strips["length"].sum()) == int(rects["size"].astype(np.int64).prod(axis=1).sum()), label
    if len(rects):
        normal = rects["size"][np.arange(len(rects)), rects["face"] // 2]
        assert (normal == 1).all() and (rects["size"] >= 1).all(), label
        assert (rects["voxel"] >= np.array(box[0])).all() and (rects["voxel"] + rects["size"] <= np.array(box[1])).all(), f"{label}: a rectangle leaves the box"
        key = np.stack([rects["voxel"][:, 0], rects["voxel"][:, 2], rects["face"], -(rects["voxel"][:, 1] + rects["size"][:, 1])], axis=1).tolist()
        assert key == sorted(key), f"{label}: not in the order of the contract"


def check_call(rules, tmp_path, solid, colour, ws, box_min, box_max, solid_outside, flags, label=""):
    want, want_summary = model.rects(solid, colour, box_min, box_max, solid_outside, flags)
    summary, rects = run_world(rules, tmp_path, ws, box_min, box_max, solid_outside, flags)
    assert summary == want_summary, f"{label}: {summary} != {want_summary}"
    if rects.tobytes() != want.tobytes():
        k = int(np.argmax(rects != want))
        raise AssertionError(f"{label}: first difference at rectangle {k}: {rects[k]} != {want[k]}")
    strips, _ = surfacemodel.surface(solid, colour, box_min, box_max, solid_outside, flags)
    lo = np.maximum(np.array(box_min), 0)
    hi = np.minimum(np.array(box_max), np.array(solid.shape))
    check_properties(rects, summary, strips, flags, (lo, hi), label)
    return rects, summary


# ---- random worlds -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("density,colours,seed", [(0.15, 2, 1), (0.4, 3, 2), (0.55, 2, 3), (0.8, 3, 4), (0.97, 2, 5)])
def test_random_worlds_equal_the_model(rules, tmp_path, density, colours, seed):
    dims = (16, 16, 8)  # (the sides of a world are powers of two)
    rng = np.random.default_rng(seed)
    solid = rng.random(dims) < density
    colour = np.where(solid, 0xFF000040 + rng.integers(0, colours, dims), 0).astype(np.uint32)
    ws = built_world(dims, solid, colour)
    try:
        merged = 0
        boxes = [((0, 0, 0), dims), ((1, 1, 1), (15, 15, 7)), ((-3, 2, 4), (7, 30, 20)), ((5, 0, 0), (6, 16, 8)), ((0, 4, 0), (16, 5, 8)), ((2, 0, 6), (13, 11, 7))]
        for k, (box_min, box_max) in enumerate(boxes):
            for flags in (0, IGNORE):
                for solid_outside in ((0x04, 0, 0x3F) if k < 2 else (0x04, 0x2A)):
                    _, summary = check_call(rules, tmp_path, solid, colour, ws, box_min, box_max, solid_outside, flags,
                                            label=f"box {box_min} .. {box_max}, outside 0x{solid_outside:02x}, flags {flags}")
                    merged += summary["strips"] - summary["rects"]
        assert merged > 100, "nothing to merge in these worlds"
    finally:
        ws.close()


# ---- constructed worlds ---------------------------------------------------------------------------------------------------------------------------

def slab_world(offset=(0, 0, 0), dims=SLAB_DIMS):
    solid = np.zeros(dims, dtype=bool)
    lo, hi = [[SLAB[k][a] + offset[a] for a in range(3)] for k in range(2)]
    solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    return solid, np.where(solid, 0xFF336699, 0).astype(np.uint32), (lo, hi)


def slab_sizes(rects):
    return {int(r["face"]): tuple(int(v) for v in r["size"]) for r in rects}


SLAB_SIZES = {0: (1, 3, 70), 1: (1, 3, 70), 2: (130, 1, 70), 3: (130, 1, 70), 4: (130, 3, 1), 5: (130, 3, 1)}


def test_the_slab_is_six_rectangles(rules, tmp_path):
    solid, colour, _ = slab_world()
    ws = built_world(SLAB_DIMS, solid, colour)
    try:
        for flags in (IGNORE, 0):
            rects, summary = check_call(rules, tmp_path, solid, colour, ws, (0, 0, 0), SLAB_DIMS, 0x04, flags, label=f"the slab, flags {flags}")
            assert summary == {"rects": 6, "strips": 18600, "unitFaces": 2 * (130 * 70 + 3 * 70 + 130 * 3), "rectsPerFace": [1] * 6}
            assert slab_sizes(rects) == SLAB_SIZES
            assert [tuple(v) for v in rects["voxel"].tolist()] == [(10, 5, 3), (10, 5, 3), (10, 7, 3), (10, 5, 3), (10, 5, 72), (139, 5, 3)]
    finally:
        ws.close()


def test_a_checkerboard_merges_only_without_colours(rules, tmp_path):
    dims = (16, 16, 16)
    x, y, z = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    solid = (x >= 2) & (x < 11) & (y >= 3) & (y < 9) & (z >= 1) & (z < 8)  # a 9 x 6 x 7 block
    colour = np.where(solid, np.where((x + y + z) % 2 == 0, 0xFF0000FF, 0xFF00FF00), 0).astype(np.uint32)
    ws = built_world(dims, solid, colour)
    try:
        area = 2 * (9 * 6 + 6 * 7 + 9 * 7)
        rects, summary = check_call(rules, tmp_path, solid, colour, ws, (0, 0, 0), dims, 0, 0, label="checkerboard")
        assert summary["rects"] == summary["strips"] == summary["unitFaces"] == area and (rects["size"] == 1).all()
        rects, summary = check_call(rules, tmp_path, solid, colour, ws, (0, 0, 0), dims, 0, IGNORE, label="checkerboard, colours ignored")
        assert summary["rects"] == 6 and summary["unitFaces"] == area
        assert slab_sizes(rects) == {0: (1, 6, 7), 1: (1, 6, 7), 2: (9, 1, 7), 3: (9, 1, 7), 4: (9, 6, 1), 5: (9, 6, 1)}
    finally:
        ws.close()


def l_floor():
    """Two floors at one height that meet in an L: x 4..23 over z 2..9, x 4..11 over z 10..21, one voxel thick, one colour."""
    dims = (32, 32, 32)
    solid = np.zeros(dims, dtype=bool)
    solid[4:24, 3, 2:10] = True
    solid[4:12, 3, 10:22] = True
    return dims, solid, np.where(solid, 0xFFA0A0A0, 0).astype(np.uint32)


def test_rows_of_different_lengths_do_not_stack(rules, tmp_path):
    dims, solid, colour = l_floor()
    ws = built_world(dims, solid, colour)
    try:
        rects, summary = check_call(rules, tmp_path, solid, colour, ws, (0, 0, 0), dims, 0, 0, label="the L")
        top = rects[rects["face"] == 3]
        assert sorted(zip(map(tuple, top["voxel"].tolist()), map(tuple, top["size"].tolist()))) == [((4, 3, 2), (20, 1, 8)), ((4, 3, 10), (8, 1, 12))]
        assert summary["rectsPerFace"][2] == 2 and summary["rectsPerFace"][3] == 2
    finally:
        ws.close()


def test_a_box_cut_in_two_tiles(rules, tmp_path):
    solid, colour, _ = slab_world()
    ws = built_world(SLAB_DIMS, solid, colour)
    try:
        cut = 77
        whole, _ = check_call(rules, tmp_path, solid, colour, ws, (0, 0, 0), SLAB_DIMS, 0x04, 0, label="whole")
        left, _ = check_call(rules, tmp_path, solid, colour, ws, (0, 0, 0), (cut, 16, 128), 0x04, 0, label="left")
        right, _ = check_call(rules, tmp_path, solid, colour, ws, (cut, 0, 0), SLAB_DIMS, 0x04, 0, label="right")
        assert rows(model.unit_faces(np.concatenate([left, right]))) == rows(model.unit_faces(whole))
        assert (left["voxel"][:, 0] + left["size"][:, 0] <= cut).all() and (right["voxel"][:, 0] >= cut).all()
        assert len(left) == 5 and len(right) == 5  # the cut faces are not exposed: the slab goes on across the seam
    finally:
        ws.close()


# ---- cvx_surface_rect_triangles -------------------------------------------------------------------------------------------------------------------

def _noise():
    dims = (12, 10, 9)  # (the model alone: no world is built)
    rng = np.random.default_rng(77)
    solid = rng.random(dims) < 0.6
    return dims, solid, np.where(solid, 0xFF102030 + rng.integers(0, 2, dims) * 0x01010100, 0).astype(np.uint32)


def test_triangles_of_single_strips_equal_the_quads_triangles():
    dims, solid, colour = _noise()
    quads, _ = surfacemodel.surface(solid, colour, (0, 0, 0), dims, 0, 0)
    assert len(quads) > 300 and (quads["length"] > 1).any()
    rects = np.zeros(len(quads), dtype=gpu.SURFACE_RECT_DTYPE)
    rects["voxel"], rects["face"], rects["argb"] = quads["voxel"], quads["face"], quads["argb"]
    rects["size"] = 1
    rects["size"][:, 1] = quads["length"]
    vertices, indices = gpu.surface_rect_triangles(rects)
    want_vertices, want_indices = gpu.surface_triangles(quads)
    assert vertices.tobytes() == want_vertices.tobytes() and indices.tobytes() == want_indices.tobytes()


def test_triangles_point_outward_and_their_areas_sum_to_the_unit_faces():
    dims, solid, colour = _noise()
    rects, summary = model.rects(solid, colour, (0, 0, 0), dims, 0, IGNORE)
    assert summary["rects"] < summary["strips"] and (rects["size"].prod(axis=1) > 4).any()
    vertices, indices = gpu.surface_rect_triangles(rects)
    assert vertices.shape == (4 * len(rects),) and indices.reshape(-1, 6).tolist() == [[4 * k + o for o in (0, 1, 2, 0, 2, 3)] for k in range(len(rects))]
    assert (vertices["uv"] == 0).all() and (vertices["material"] == -1).all()
    total = 0.0
    for k, r in enumerate(rects):
        axis, up = int(r["face"]) // 2, int(r["face"]) % 2
        p = vertices["position"][4 * k:4 * k + 4].astype(np.float64)
        assert (p[:, axis] == r["voxel"][axis] + up).all(), (k, p)
        lo = r["voxel"].astype(np.float64)
        hi = lo + r["size"]
        others = [a for a in range(3) if a != axis]
        assert sorted(map(tuple, p[:, others].tolist())) == sorted((u, v) for u in (lo[others[0]], hi[others[0]]) for v in (lo[others[1]], hi[others[1]]))
        outward = np.zeros(3)
        outward[axis] = 1 if up else -1
        for a, b, c in ((0, 1, 2), (0, 2, 3)):
            n = np.cross(p[b] - p[a], p[c] - p[a])
            assert np.dot(n, outward) > 0 and not n[others].any(), (k, n)
            total += np.linalg.norm(n) / 2
        word = int(r["argb"])
        assert vertices["rgba"][4 * k:4 * k + 4].tolist() == [[(word >> 8) & 0xFF, (word >> 16) & 0xFF, word >> 24, 255]] * 4
    assert total == summary["unitFaces"]
    empty_v, empty_i = gpu.surface_rect_triangles(np.zeros(0, dtype=gpu.SURFACE_RECT_DTYPE))
    assert len(empty_v) == 0 and len(empty_i) == 0
    bad = rects[:1].copy()
    bad["size"][0, int(bad["face"][0]) // 2] = 2
    with pytest.raises(gpu.CvxError, match="size"):
        gpu.surface_rect_triangles(bad)


# ---- layouts and entry points ------------------------------------------------------------------------------------------------------------------

def test_the_calls_fail_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(8, 8, 8)
    ms = C.c_float()
    for entry in (L.cvx_world_surface_rects, L.cvx_world_surface_rects_device):
        assert entry(None, lo, hi, gpu.SURFACE_OUTSIDE_DEFAULT, 0, None, 0, None, C.byref(ms)) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    # a context without a device (tests/surface_rects_rules.cpp): every bad argument of both calls, then CVX_ERR_NOT_READY without a world, a box
    # outside an uploaded world, and cvx_surface_rect_triangles' own checks
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 16 + [-3, -3] + [-1, -1] + [-1] * 8 + [0, 0], codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_surface_rects(h, lo, hi, gpu.SURFACE_OUTSIDE_DEFAULT, 0, None, 0, None, C.byref(ms)) == -3
        finally:
            L.cvx_destroy(h)
