"""Models and fixtures for the mesh-stamp tests (tests/test_world_stamp_cpu.py, tests/test_gpu_world_stamp.py,
tests/test_gpu_world_stamp_limits.py).

- rules(): tests/stamp_rules.cpp compiled with g++ against cpuvox_amd/csrc/cvx_stamp.h (the rules the device runs).
- voxelise(): a host.Mesh through the triangle rule, triangle after triangle: (x, y, z, argb) in emission order.
- counts() / hits(): what the device's pipeline makes of every triangle (pairs, hits, kept hits, ...) and the hits themselves, uncapped.
- apply_stamp(): a dense (solid, colour) volume after stamping voxels with FILL / CARVE / PAINT, duplicates merged with ToFinalColumn's
  average (per channel sum // count, alpha 255).
- write_obj() / write_tga(): meshes and textures as files, for host.Mesh.from_obj and host.WorldSet.from_obj."""
import lzma
import os
import struct
import subprocess

import numpy as np

import ruleslib
from cpuvox_amd import gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def rules(tmpdir) -> str:
    return ruleslib.build("stamp_rules", tmpdir)


def mill_obj(tmpdir) -> str:
    """tests/golden/mill.obj.xz (the reference's datasets/mill.obj) unpacked into tmpdir."""
    path = os.path.join(str(tmpdir), "mill.obj")
    if not os.path.exists(path):
        with lzma.open(os.path.join(GOLDEN, "mill.obj.xz")) as src, open(path, "wb") as dst:
            dst.write(src.read())
    return path


def _mesh_file(mesh, dims, tmpdir) -> str:
    """The mesh in the layout tests/stamp_rules.cpp reads."""
    v, idx = mesh.vertices, mesh.indices
    parts = [struct.pack("<6i", dims[0], dims[1], dims[2], v.size, idx.size, mesh.material_count), v.tobytes(), idx.astype("<i4").tobytes()]
    for k in range(mesh.material_count):
        t = mesh.texture(k)
        if t is None:
            parts.append(struct.pack("<2i", 0, 0))
        else:
            parts.append(struct.pack("<2i", t.shape[1], t.shape[0]) + t.tobytes())
    src = os.path.join(str(tmpdir), "mesh.bin")
    with open(src, "wb") as f:
        f.write(b"".join(parts))
    return src


def voxelise(binary, mesh, dims, tmpdir):
    """(x, y, z, argb) arrays of what the triangle rule emits for every triangle of `mesh` in a world of `dims`, in emission order."""
    src, dst = _mesh_file(mesh, dims, tmpdir), os.path.join(str(tmpdir), "voxels.bin")
    subprocess.check_call([binary, "voxelise", src, dst])
    w = np.fromfile(dst, dtype="<u4").reshape(-1, 4)
    return w[:, 0].astype(np.int32), w[:, 1].astype(np.int32), w[:, 2].astype(np.int32), w[:, 3].copy()


COUNTS_DTYPE = np.dtype([("pairs", "<i4"), ("hits", "<i4"), ("kept", "<i4"), ("opaque", "<i4"), ("column_max", "<i4"), ("midpair", "<i4")])


def counts(binary, mesh, dims, tmpdir):
    """Per triangle of `mesh`, what the device's pipeline makes of it (cvx_stamp.hip; the rule's `counts` mode): the columns of its box (the
    device's pairs), its hits, the hits kept under the per-triangle cap, the opaque ones among those, the most hits in one column and whether
    the cap falls strictly inside a column.  A COUNTS_DTYPE array."""
    src, dst = _mesh_file(mesh, dims, tmpdir), os.path.join(str(tmpdir), "counts.bin")
    subprocess.check_call([binary, "counts", src, dst])
    out = np.fromfile(dst, dtype=COUNTS_DTYPE)
    assert len(out) == mesh.indices.size // 3
    return out


def hits(binary, mesh, dims, tmpdir):
    """Every hit of every triangle in the host's loop order, the ones past the cap and the transparent ones included: (triangle, x, y, z)
    arrays.  A triangle's first 262144 are the ones it keeps."""
    src, dst = _mesh_file(mesh, dims, tmpdir), os.path.join(str(tmpdir), "hits.bin")
    subprocess.check_call([binary, "hits", src, dst])
    w = np.fromfile(dst, dtype="<i4").reshape(-1, 4)
    return w[:, 0], w[:, 1], w[:, 2], w[:, 3]


def merge(x, y, z, argb):
    """Unique voxels (x, y, z) and their merged colours."""
    if len(x) == 0:
        e = np.zeros(0, dtype=np.int64)
        return e, e, e, np.zeros(0, dtype=np.uint32)
    keys = np.stack([np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(z, np.int64)], axis=1)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.ravel()
    count = np.bincount(inv, minlength=len(uniq))
    out = np.full(len(uniq), 0xFF, dtype=np.uint32)
    for shift in (8, 16, 24):
        s = np.bincount(inv, weights=((argb >> shift) & 0xFF).astype(np.float64), minlength=len(uniq)).astype(np.int64)
        out |= ((s // count).astype(np.uint32) << shift)
    return uniq[:, 0], uniq[:, 1], uniq[:, 2], out


def apply_stamp(solid, colour, x, y, z, argb, op):
    """The dense volume after stamping (in place)."""
    ux, uy, uz, c = merge(x, y, z, argb)
    if op == gpu.BRUSH_FILL:
        solid[ux, uy, uz] = True
        colour[ux, uy, uz] = c
    elif op == gpu.BRUSH_CARVE:
        solid[ux, uy, uz] = False
        colour[ux, uy, uz] = 0
    else:
        keep = solid[ux, uy, uz]
        colour[ux[keep], uy[keep], uz[keep]] = c[keep]
    return solid, colour


def write_tga(path, rgba):
    """rgba: uint8 [H, W, 4], row 0 = the bottom row -> an uncompressed 32-bit TGA stored bottom-up."""
    h, w, _ = rgba.shape
    head = struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, w, h, 32, 8)
    bgra = rgba[:, :, [2, 1, 0, 3]]
    with open(path, "wb") as f:
        f.write(head + bgra.tobytes())


def write_obj(path, positions, colours=None, faces=(), uvs=None, face_uvs=None, materials=None, face_materials=None):
    """An OBJ the host importer reads: `v x y z [r g b]`, `vt u v`, `f a/t b/t c/t` (1-based), `usemtl` per face when face_materials is given
    (materials: {name: texture path or None}, written to a .mtl next to it)."""
    lines = []
    if materials:
        mtl = os.path.splitext(path)[0] + ".mtl"
        with open(mtl, "w") as f:
            for name, tex in materials.items():
                f.write(f"newmtl {name}\n")
                if tex is not None:
                    f.write(f"map_Kd {os.path.basename(tex)}\n")
        lines.append(f"mtllib {os.path.basename(mtl)}")
    for i, p in enumerate(positions):
        if colours is not None:
            c = colours[i]
            lines.append(f"v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r} {float(c[0])!r} {float(c[1])!r} {float(c[2])!r}")
        else:
            lines.append(f"v {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}")
    if uvs is not None:
        for u in uvs:
            lines.append(f"vt {float(u[0])!r} {float(u[1])!r}")
    current = None
    for k, f in enumerate(faces):
        if face_materials is not None and face_materials[k] != current:
            current = face_materials[k]
            lines.append(f"usemtl {current}")
        if face_uvs is not None:
            t = face_uvs[k]
            lines.append(f"f {f[0] + 1}/{t[0] + 1} {f[1] + 1}/{t[1] + 1} {f[2] + 1}/{t[2] + 1}")
        else:
            lines.append(f"f {f[0] + 1} {f[1] + 1} {f[2] + 1}")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return path
