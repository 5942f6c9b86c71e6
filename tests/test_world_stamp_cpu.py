"""CPU (no GPU needed): the rules behind cvx_world_stamp_mesh (cpuvox_amd/csrc/cvx_stamp.h), compiled for the host through tests/stamp_rules.cpp.

- The triangle rule against the host voxeliser: meshes written as OBJ files (random triangles, slivers and zero-area triangles, triangles partly
  outside the world, textured quads with transparent texels, negative and out-of-range material indices, one triangle over the 262144-hit
  cap) go through host.Mesh.from_obj(...).rescale(...) and the rule; the emitted voxels, built with tests/pyworld.py's build_lod0 (which
  averages duplicates itself), must equal host.WorldSet.from_obj of the same file byte for byte.
- The column rule StampColumn (with MergeStamped) against a dense numpy model on thousands of random columns: all three ops, duplicates and
  over-limit columns.
- The layouts of cvx_mesh_vertex / cvx_mesh_texture across C, ctypes, numpy and C#; the mesh API round trip; the new call without a context /
  world."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pyworld
import ruleslib
import stampmodel
from cpuvox_amd import gpu, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("stamp")
    return d, stampmodel.rules(d)


# ---- the triangle rule against the host voxeliser -------------------------------------------------------------------------------------------

def _random_triangles(rng, count, spread=1.0, size=0.2):
    centres = rng.uniform(-spread, spread, size=(count, 3))
    return (centres[:, None, :] + rng.normal(0.0, size, size=(count, 3, 3))).reshape(-1, 3)


def _slivers(rng, count):
    """Needles, triangles with repeated or collinear corners and near-degenerate ones (NaN barycentrics on the host)."""
    out = []
    for k in range(count):
        a = rng.uniform(-1, 1, size=3)
        d = rng.normal(size=3)
        kind = k % 4
        if kind == 0:
            tri = [a, a + d, a + d * (1 + 1e-7)]
        elif kind == 1:
            tri = [a, a, a + d]
        elif kind == 2:
            tri = [a, a + d, a + 2 * d]
        else:
            tri = [a, a + d * 1e-6, a + rng.normal(size=3) * 1e-6]
        out.extend(tri)
    return np.array(out)


def _check_obj(work, path, max_dimension, flip=(True, False, False)):
    d, rules = work
    mesh = host.Mesh.from_obj(path)
    dims = mesh.rescale(max_dimension, flip)
    x, y, z, argb = stampmodel.voxelise(rules, mesh, dims, d)
    level = pyworld.build_lod0(dims, zip(x.tolist(), y.tolist(), z.tolist(), argb.tolist()))
    ws = host.WorldSet.from_obj(path, max_dimension, flip=flip)
    assert tuple(ws.dims) == tuple(dims)
    assert level.blob() == ws.storage(0).tobytes()
    return len(x)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_triangles_equal_the_host_voxeliser(work, tmp_path, seed):
    rng = np.random.default_rng(seed)
    pos = np.concatenate([_random_triangles(rng, 60), _slivers(rng, 24)])
    colours = rng.uniform(-0.1, 1.1, size=(len(pos), 3))
    faces = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(pos) // 3)]
    path = stampmodel.write_obj(str(tmp_path / "tri.obj"), pos, colours, faces)
    assert _check_obj(work, path, 64) > 500


def test_triangles_partly_outside_the_world(work, tmp_path):
    """Rescale fits the mesh to the world, so a second pass with a flip and a non-power-of-two extent puts parts of triangles past the box:
    the host clamps, and so does the rule."""
    rng = np.random.default_rng(5)
    pos = _random_triangles(rng, 40, spread=1.0, size=0.5)
    pos[:3] = [[-1.0, -1.0, -1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, 1.0]]  # the extent: a box around the others
    faces = [(3 * k, 3 * k + 1, 3 * k + 2) for k in range(len(pos) // 3)]
    path = stampmodel.write_obj(str(tmp_path / "out.obj"), pos, rng.uniform(0, 1, size=(len(pos), 3)), faces)
    _check_obj(work, path, 48, flip=(True, True, False))
    d, rules = work
    mesh = host.Mesh.from_obj(path)
    dims = mesh.rescale(48, (True, True, False))
    v = mesh.vertices
    assert (v["position"].max(axis=0) > np.array(dims) - 1).any(), "some triangle must reach past the world's last voxel"


def test_textured_quads_and_material_indices(work, tmp_path):
    rng = np.random.default_rng(9)
    tex = rng.integers(0, 256, size=(12, 10, 4)).astype(np.uint8)
    tex[..., 3] = np.where(rng.random((12, 10)) < 0.35, rng.integers(0, 255, size=(12, 10)), 255)
    stampmodel.write_tga(str(tmp_path / "tex.tga"), tex)
    pos = np.array([[0, 0, 0], [1, 0, 0], [1, 0.3, 1], [0, 0.3, 1],      # quad, textured
                    [0, 0.6, 0], [1, 0.6, 0], [1, 1, 1], [0, 1, 1],      # quad, material without a texture
                    [0.2, 0.1, 0.1], [0.9, 0.8, 0.2], [0.1, 0.9, 0.9],   # triangle, no material (-1)
                    [0.3, 0.2, 0.5], [0.7, 0.5, 0.8], [0.2, 0.7, 0.3]], dtype=np.float64)
    uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [-0.5, 2.0], [1.5, -1.0]])
    faces = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7), (8, 9, 10), (11, 12, 13)]
    face_uvs = [(0, 1, 2), (0, 2, 3), (0, 1, 2), (0, 2, 3), (0, 1, 2), (4, 5, 0)]
    mats = ["tex", "tex", "plain", "plain", "none", "tex"]  # "none" is not in the library: material -1
    path = stampmodel.write_obj(str(tmp_path / "tex.obj"), pos, rng.uniform(0, 1, size=(len(pos), 3)), faces, uvs, face_uvs,
                                {"tex": str(tmp_path / "tex.tga"), "plain": None}, mats)
    n = _check_obj(work, path, 64)
    assert n > 500
    mesh = host.Mesh.from_obj(path)
    assert mesh.material_count == 2 and mesh.texture(1) is None
    assert np.array_equal(mesh.texture(0), tex)
    assert sorted(set(mesh.vertices["material"].tolist())) == [-1, 0, 1]


def test_material_indices_as_int8(work):
    """(sbyte)v0.material: 256 addresses material 0; 200 (-56), -1 and 7 (out of range) mean no texture: the vertex colour alone."""
    d, rules = work
    rng = np.random.default_rng(12)
    tex = rng.integers(0, 256, size=(4, 4, 4)).astype(np.uint8)
    tex[..., 3] = np.where(rng.random((4, 4)) < 0.3, 100, 255)
    pos = np.float32([[2, 2, 2], [28, 9, 2], [2, 20, 28]])

    def voxels(material):
        mesh = host.Mesh.from_arrays({"position": pos, "rgba": [[10, 200, 30, 255], [200, 10, 30, 255], [30, 10, 200, 255]],
                                      "uv": np.float32([[0, 0], [1, 0], [0, 1]]), "material": material}, textures=[tex])
        return np.stack(stampmodel.voxelise(rules, mesh, (32, 32, 32), d))

    textured, untextured = voxels(0), voxels(-1)
    assert textured.shape[1] < untextured.shape[1], "transparent texels emit no voxel"
    assert np.array_equal(voxels(256), textured)
    for m in (200, 7, -129 + 256 * 3):
        assert np.array_equal(voxels(m), untextured), m


def test_cap_triangle_equals_the_host_voxeliser(work, tmp_path):
    """One triangle whose box holds more than 262144 hits: the host stops at the cap, in x, z, y order, and so does the rule."""
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 0.002, 1], [0.2, 0.0005, 0.2], [0.21, 0.0005, 0.2], [0.2, 0.0006, 0.21]])
    path = stampmodel.write_obj(str(tmp_path / "cap.obj"), pos, np.full((6, 3), 0.5), [(0, 1, 2), (3, 4, 5)])
    d, rules = work
    mesh = host.Mesh.from_obj(path)
    dims = mesh.rescale(1024)
    x, y, z, argb = stampmodel.voxelise(rules, mesh, dims, d)
    assert len(x) >= 262144
    ws = host.WorldSet.from_obj(path, 1024)
    assert host.WorldSet.from_voxels(dims, x, y, z, argb).storage(0).tobytes() == ws.storage(0).tobytes()


def test_mill_equals_the_host_voxeliser(work):
    d, rules = work
    obj = stampmodel.mill_obj(d)
    mesh = host.Mesh.from_obj(obj)
    dims = mesh.rescale(128)
    x, y, z, argb = stampmodel.voxelise(rules, mesh, dims, d)
    ws = host.WorldSet.from_obj(obj, 128)
    mine = host.WorldSet.from_voxels(dims, x, y, z, argb)
    for k in range(6):
        assert mine.storage(k).tobytes() == ws.storage(k).tobytes(), f"LOD {k}"


def test_counts_and_hits_modes_agree_with_the_voxeliser(work):
    """stamp_rules counts / hits (what tests/test_gpu_world_stamp_limits.py names its cases after) on the three triangles that file is built
    around, a triangle without area and a textured one: the figures, and hits == VoxelizeTriangle's voxels up to the cap."""
    d, rules = work
    f = np.float32
    wall = [[10.3, 2, 10.2], [10.9, 60, 50.1], [11.4, 3, 52.7]]
    ramp = np.float32([[0.2, 1.3, 0.4], [127.6, f(1.3) + f(36) * f(127.4), 3.1], [2.7, 9.9, 127.2]])
    tall = [[3.5, -1, 3.2], [3.5, 100000, 5.0], [3.5, -1, 6.9]]
    for tri, dims, want in ((wall, (128, 64, 128), (138, 1255, 1255, 1255, 45, 0)), (ramp, (128, 8192, 128), (16384, 290965, 262144, 262144, 37, 1)),
                            (tall, (32, 32768, 32), (10, 103256, 103256, 103256, 32768, 0))):
        mesh = host.Mesh.from_arrays({"position": np.float32([[1, 1, 1], [1, 1, 1], [5, 5, 5]] + [list(p) for p in tri])})
        c = stampmodel.counts(rules, mesh, dims, d)
        assert c[0].tolist() == (0, 0, 0, 0, 0, 0) and c[1].tolist() == want, c
        t, hx, hy, hz = stampmodel.hits(rules, mesh, dims, d)
        x, y, z, _ = stampmodel.voxelise(rules, mesh, dims, d)
        assert len(t) == want[1] and (t == 1).all() and len(x) == want[2]
        assert np.array_equal(hx[:len(x)], x) and np.array_equal(hy[:len(x)], y) and np.array_equal(hz[:len(x)], z)
    rng = np.random.default_rng(21)
    tex = rng.integers(0, 256, size=(8, 8, 4)).astype(np.uint8)
    tex[..., 3] = np.where(rng.random((8, 8)) < 0.4, 17, 255)
    mesh = host.Mesh.from_arrays({"position": np.float32(wall), "uv": np.float32([[0, 0], [1, 0], [0, 1]]), "material": 0}, textures=[tex])
    c = stampmodel.counts(rules, mesh, (128, 64, 128), d)[0]
    assert c["kept"] == 1255 and 0 < c["opaque"] < 1255 and c["opaque"] == len(stampmodel.voxelise(rules, mesh, (128, 64, 128), d)[0])


# ---- the column rule --------------------------------------------------------------------------------------------------------------------------

def _random_column(rng, dim_y):
    solid = np.zeros(dim_y, dtype=bool)
    for _ in range(int(rng.integers(0, 5))):
        lo = int(rng.integers(0, dim_y))
        solid[lo:lo + int(rng.integers(1, max(2, dim_y // 3)))] = True
    ys = np.nonzero(solid)[0][::-1]
    cols = rng.integers(0, 2**32, size=len(ys), dtype=np.uint64).astype(np.uint32)
    col = pyworld.final_column([(int(y), int(c)) for y, c in zip(ys, cols)], dim_y - 1, 1)
    dense = np.zeros(dim_y, dtype=np.uint32)
    if col is None:
        return [], [], solid, dense
    runs, colours, _, _ = col
    top = dim_y
    for ci, n in runs:
        if ci >= 0:
            for i in range(n):
                dense[top - 1 - i] = colours[ci + i]
        top -= n
    return list(runs), list(colours), solid, dense


def test_stamp_column_rule_against_a_dense_model(work, tmp_path):
    d, rules = work
    rng = np.random.default_rng(2024)
    cases, expect = [], []
    for k in range(3000):
        big = k % 50 == 0
        dim_y = int(rng.choice([8, 33, 64, 256])) if not big else 65536
        runs, colours, solid, dense = _random_column(rng, dim_y) if not big else ([], [], np.zeros(dim_y, bool), np.zeros(dim_y, np.uint32))
        op = int(rng.integers(0, 3))
        if big:  # over the limits: a stamped voxel every other y gives more than 32767 runs of length 1 / colours past index 32767
            ys = np.arange(0, dim_y, 2)
            op = gpu.BRUSH_FILL
        else:
            ys = rng.integers(0, dim_y, size=int(rng.integers(0, dim_y)))
        vc = rng.integers(0, 2**32, size=len(ys), dtype=np.uint64).astype(np.uint32)
        stride = int(rng.choice([1, 32]))
        base = int(rng.integers(1, 50))  # (colorsBase 0 is never a column's: the arena starts with a line of zeros)
        words = [dim_y, stride] + ruleslib.column_words(base, runs, colours) + [op, len(ys)]
        for y, c in zip(ys, vc):
            words += [int(y), int(c)]
        cases.append(struct.pack(f"<{len(words)}I", *[w & 0xFFFFFFFF for w in words]))
        # the model
        s, col = solid.copy(), dense.copy()
        ux, uy, uz, uc = stampmodel.merge(np.zeros(len(ys), np.int64), ys, np.zeros(len(ys), np.int64), vc)
        if op == gpu.BRUSH_FILL:
            s[uy], col[uy] = True, uc
        elif op == gpu.BRUSH_CARVE:
            s[uy] = False
        else:
            keep = s[uy]
            col[uy[keep]] = uc[keep]
        vox = [(int(y), int(col[y])) for y in np.nonzero(s)[0][::-1]]
        expect.append(pyworld.final_column(vox, dim_y - 1, 1) if vox else None)
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    open(src, "wb").write(b"".join(cases))
    subprocess.check_call([rules, "stamp", src, dst])
    out = np.fromfile(dst, dtype="<u4")
    at, over = 0, 0
    for k, want in enumerate(expect):
        flag, run_count, n_col, wmin, wmax = (int(v) for v in out[at:at + 5])
        at += 5
        if flag:
            over += 1
            assert want is not None and (len(want[0]) > 65535 or max(n for _, n in want[0]) > 32767 or
                                         max(ci for ci, _ in want[0]) > 32767), f"case {k}: flagged, but the column fits"
            continue
        if want is None:
            assert run_count == 0 and n_col == 0, f"case {k}"
            continue
        runs = out[at:at + run_count]
        at += run_count
        colours = out[at:at + n_col]
        at += n_col
        got_runs = [((int(r) & 0xFFFF) if (int(r) & 0xFFFF) != 0xFFFF else -1, int(r) >> 16) for r in runs]
        assert got_runs == [(ci, n) for ci, n in want[0]], f"case {k}: runs"
        assert colours.tolist() == [int(c) for c in want[1]], f"case {k}: colours"
        assert (wmin, wmax) == (want[2], want[3]), f"case {k}: worldMin / worldMax"
    assert at == len(out)
    assert over >= 50, "the over-limit columns must be flagged"


# ---- layouts, the mesh API and the call without a world -----------------------------------------------------------------------------------------

def test_struct_layouts_match_across_c_ctypes_numpy_and_csharp():
    header = open(os.path.join(ROOT, "include", "cpuvox_gpu.h")).read()
    assert re.search(r"typedef struct cvx_mesh_vertex \{ /\* 28 bytes \*/\s*float position\[3\];.*?uint8_t rgba\[4\];.*?float uv\[2\];.*?int32_t material;", header, re.S)
    assert re.search(r"typedef struct cvx_mesh_texture \{ /\* 16 bytes \*/\s*int32_t width, height;\s*const uint8_t \*rgba;", header, re.S)
    assert C.sizeof(host.MeshVertex) == 28 and host.MeshVertex.rgba.offset == 12 and host.MeshVertex.uv.offset == 16 and host.MeshVertex.material.offset == 24
    assert C.sizeof(host.MeshTexture) == 16 and host.MeshTexture.rgba.offset == 8
    assert gpu.MESH_VERTEX_DTYPE == host.MESH_VERTEX_DTYPE and gpu.MESH_VERTEX_DTYPE.itemsize == 28
    assert [gpu.MESH_VERTEX_DTYPE.fields[f][1] for f in ("position", "rgba", "uv", "material")] == [0, 12, 16, 24]
    cs = open(os.path.join(ROOT, "host", "csharp", "CpuVoxGpu.cs")).read()
    m = re.search(r"public unsafe struct MeshVertex\s*\{(.*?)\n\t\}", cs, re.S)
    assert m and re.findall(r"(Position\[3\]|Rgba\[4\]|Uv\[2\]|int Material)", m.group(1)) == ["Position[3]", "Rgba[4]", "Uv[2]", "int Material"]
    m = re.search(r"public unsafe struct MeshTexture\s*\{(.*?)\n\t\}", cs, re.S)
    assert m and "int Width, Height;" in m.group(1) and "byte* Rgba;" in m.group(1)
    for name in ("cvxh_mesh_load_obj", "cvxh_mesh_create", "cvxh_mesh_rescale", "cvxh_mesh_vertices", "cvxh_mesh_indices", "cvxh_mesh_material_count",
                 "cvxh_mesh_texture", "cvxh_mesh_free"):
        assert re.search(r"\[DllImport\(HostLib\)\] public static extern \w+\*? " + name + r"\(", cs), name


def test_mesh_api_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    v = np.zeros(6, dtype=gpu.MESH_VERTEX_DTYPE)
    v["position"] = rng.uniform(-3, 5, size=(6, 3))
    v["rgba"] = rng.integers(0, 256, size=(6, 4))
    v["uv"] = rng.uniform(0, 1, size=(6, 2))
    v["material"] = [0, 0, 0, 1, 1, -1]
    tex = rng.integers(0, 256, size=(3, 5, 4)).astype(np.uint8)
    m = host.Mesh.from_arrays(v, [0, 1, 2, 3, 4, 5], [tex, None])
    assert m.vertices.tobytes() == v.tobytes() and m.indices.tolist() == list(range(6))
    assert m.material_count == 2 and np.array_equal(m.texture(0), tex) and m.texture(1) is None
    dims = m.rescale(32)
    p = m.vertices["position"]
    ext = v["position"].max(axis=0) - v["position"].min(axis=0)
    scale = np.float32(32) / np.float32(ext.max())
    assert dims == tuple(1 << int(np.ceil(np.log2(max(1, int(e * scale))))) for e in ext)
    assert np.allclose(p[:, 0], dims[0] - (v["position"][:, 0] - v["position"][:, 0].min()) * scale, atol=1e-4)  # X flipped by default
    assert np.allclose(p[:, 1:], (v["position"][:, 1:] - v["position"].min(axis=0)[1:]) * scale, atol=1e-4)
    # an OBJ: what from_obj imports
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 1]], dtype=np.float64)
    path = stampmodel.write_obj(str(tmp_path / "one.obj"), pos, [[1, 0.5, 0]] * 3, [(0, 1, 2)])
    o = host.Mesh.from_obj(path)
    assert o.vertices["position"].tolist() == pos.tolist() and o.vertices["rgba"].tolist() == [[255, 128, 0, 255]] * 3
    assert o.vertices["material"].tolist() == [-1] * 3 and o.material_count == 0
    with pytest.raises(RuntimeError):
        host.Mesh.from_obj(str(tmp_path / "missing.obj"))
    with pytest.raises(RuntimeError):
        host.Mesh.from_arrays(v, [0, 1, 6])
    with pytest.raises(RuntimeError):
        host.Mesh.from_arrays(v, [0, 1])
    L = host.lib()
    assert L.cvxh_mesh_rescale(None, 1.0, 0, 0, 0, (C.c_int32 * 3)()) != 0
    assert L.cvxh_mesh_texture(m._h, 2, C.byref(host.MeshTexture())) != 0


def test_stamp_without_a_context_or_world_fails_cleanly(work):
    d, rules = work
    out = subprocess.run([rules, "args"], capture_output=True, text=True, check=True).stdout.split()
    codes = [int(c) for c in out]
    # no context; op; levelCount 6 / -1; indexCount 2; index 3; 129 materials; -1 materials; a texture of width 0; NaN; 3e7; valid -> no world
    assert codes == [-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -3], codes
    assert gpu.lib().cvx_world_stamp_mesh(None, None, 0, None, 0, None, 0, 0, 0, None) == -1  # CVX_ERR_INVALID_ARGUMENT
