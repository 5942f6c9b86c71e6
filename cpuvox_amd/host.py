"""ctypes binding of libcpuvox_host.so (include/cpuvox_host.h).

Thin by design: the host-side mirror of the reference's managed code (world
building, camera / vanishing point / segment setup, LOD distances, benchmark
path) lives in C++ (cpuvox_amd/csrc/host); this module only marshals.
Reference counterparts: UnityManager.cs:163-201,297-343,417-458 and
RenderManager.cs:111-152,374-510.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

LOD_LEVELS = 6  # UnityManager.cs:42

_HERE = os.path.dirname(os.path.abspath(__file__))


class SegmentData(C.Structure):
    """RenderManager.SegmentData (RenderManager.cs:503-510) == cvx_segment_data."""

    _fields_ = [
        ("MinScreen", C.c_float * 2),
        ("MaxScreen", C.c_float * 2),
        ("CamLocalPlaneRayMin", C.c_float * 2),
        ("CamLocalPlaneRayMax", C.c_float * 2),
        ("RayCount", C.c_int32),
    ]


class CameraData(C.Structure):
    """CameraData (CameraData.cs:11-16) == cvx_camera_data."""

    _fields_ = [
        ("WorldToScreenMatrix", C.c_float * 16),
        ("PositionXZ", C.c_float * 2),
        ("PositionY", C.c_float),
        ("InverseElementIterationDirection", C.c_uint8),
        ("pad_", C.c_uint8 * 3),
        ("FarClip", C.c_float),
        ("LODDistances", C.c_float * LOD_LEVELS),
    ]


class WorldInfo(C.Structure):
    _fields_ = [
        ("storage", C.c_void_p),
        ("byteLength", C.c_int64),
        ("dimX", C.c_int32),
        ("dimY", C.c_int32),
        ("dimZ", C.c_int32),
        ("lod", C.c_int32),
        ("columnCount", C.c_int32),
        ("elementCount", C.c_int64),
    ]


class CameraPose(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("eulerAngles", C.c_float * 3),
        ("fieldOfView", C.c_float),
        ("nearClipPlane", C.c_float),
        ("pixelWidth", C.c_int32),
        ("pixelHeight", C.c_int32),
    ]


class Frame(C.Structure):
    _fields_ = [
        ("segments", SegmentData * 4),
        ("camera", CameraData),
        ("vanishingPointScreenSpace", C.c_float * 2),
        ("vanishingPointWorldSpace", C.c_float * 3),
        ("forward", C.c_float * 3),
        ("totalRays", C.c_int32),
    ]


class MeshVertex(C.Structure):
    """SimpleMesh.Vertex (SimpleMesh.cs:108-114) == cvx_mesh_vertex."""

    _fields_ = [("position", C.c_float * 3), ("rgba", C.c_uint8 * 4), ("uv", C.c_float * 2), ("material", C.c_int32)]


class MeshTexture(C.Structure):
    """cvx_mesh_texture: width x height RGBA8 texels, row 0 = the bottom row; rgba NULL = no texture."""

    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgba", C.c_void_p)]


# numpy view of cvx_mesh_vertex (also cpuvox_amd.gpu.MESH_VERTEX_DTYPE)
MESH_VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("rgba", "u1", 4), ("uv", "<f4", 2), ("material", "<i4")])

assert C.sizeof(SegmentData) == 36 and C.sizeof(CameraData) == 108
assert C.sizeof(MeshVertex) == 28 and MESH_VERTEX_DTYPE.itemsize == 28 and C.sizeof(MeshTexture) == 16

_lib = None


def lib() -> C.CDLL:
    """Load libcpuvox_host.so (built in-tree by cpuvox_amd/csrc/Makefile)."""
    global _lib
    if _lib is None:
        path = os.environ.get("CVX_HOST_LIB") or os.path.join(_HERE, "libcpuvox_host.so")  # CVX_HOST_LIB: another build of the same ABI (sanitizer build in tests)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C cpuvox_amd/csrc`")
        L = C.CDLL(path)
        L.cvxh_last_error.restype = C.c_char_p
        L.cvxh_version.restype = C.c_char_p
        L.cvxh_world_lod0_voxels.restype = C.c_int64
        L.cvxh_world_extract_region.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                C.POINTER(C.c_int32)]
        L.cvxh_free.argtypes = [C.c_void_p]
        L.cvxh_world_lod0_voxels.argtypes = [C.c_void_p]
        L.cvxh_world_from_obj.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.cvxh_world_procedural.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]
        L.cvxh_world_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.cvxh_world_save.argtypes = [C.c_void_p, C.c_char_p]
        L.cvxh_world_from_blobs.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]
        L.cvxh_world_downsample_seconds.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.cvxh_world_free.argtypes = [C.c_void_p]
        L.cvxh_world_free.restype = None
        L.cvxh_world_lod_count.argtypes = [C.c_void_p]
        L.cvxh_world_info_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(WorldInfo)]
        L.cvxh_world_builder_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.cvxh_world_builder_set_voxels.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cvxh_world_builder_finish.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.cvxh_world_builder_free.argtypes = [C.c_void_p]
        L.cvxh_world_builder_free.restype = None
        L.cvxh_setup_lods.argtypes = [C.POINTER(CameraPose), C.c_int, C.c_int, C.c_int, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.cvxh_setup_lods_ex.argtypes = [C.POINTER(CameraPose), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.cvxh_setup_frame.argtypes = [C.POINTER(CameraPose), C.c_int, C.c_float, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.POINTER(Frame)]
        L.cvxh_sample_benchmark_path.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.cvxh_sample_benchmark_path.restype = None
        L.cvxh_image_load.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p, C.c_int64]
        L.cvxh_mesh_load_obj.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
        L.cvxh_mesh_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.cvxh_mesh_rescale.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        L.cvxh_mesh_vertices.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]
        L.cvxh_mesh_indices.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
        L.cvxh_mesh_material_count.argtypes = [C.c_void_p]
        L.cvxh_mesh_texture.argtypes = [C.c_void_p, C.c_int, C.POINTER(MeshTexture)]
        L.cvxh_mesh_free.argtypes = [C.c_void_p]
        L.cvxh_mesh_free.restype = None
        _lib = L
    return _lib


def default_threads() -> int:
    """Worker threads the host library uses for `threads <= 0` (cgroup-quota aware)."""
    return lib().cvxh_default_threads()


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"cpuvox_host error {rc}: {lib().cvxh_last_error().decode()}")


class WorldSet:
    """World[] worldLODs (UnityManager.cs:15): LOD_LEVELS RLE worlds kept in the
    reference's storage layout, ready for cvx_world_upload."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    # -- constructors -----------------------------------------------------
    @staticmethod
    def from_obj(path: str, max_dimension: int, swap_yz=False, flip=(True, False, False), threads=0) -> "WorldSet":
        """UnityManager 'Convert' (UnityManager.cs:297-343); default flips X (UnityManager.cs:27)."""
        h = C.c_void_p()
        _check(lib().cvxh_world_from_obj(path.encode(), max_dimension, int(swap_yz), int(flip[0]), int(flip[1]), int(flip[2]), threads, C.byref(h)))
        return WorldSet(h.value)

    @staticmethod
    def procedural(dim_x: int, dim_y: int, dim_z: int, seed: int = 0x5EED2048, threads=0) -> "WorldSet":
        h = C.c_void_p()
        _check(lib().cvxh_world_procedural(dim_x, dim_y, dim_z, seed & 0xFFFFFFFF, threads, C.byref(h)))
        return WorldSet(h.value)

    @staticmethod
    def load(path: str) -> "WorldSet":
        """WorldSaveFile.Deserialize (WorldSaveFile.cs:57)."""
        h = C.c_void_p()
        _check(lib().cvxh_world_load(path.encode(), C.byref(h)))
        return WorldSet(h.value)

    @staticmethod
    def from_voxels(dims, x, y, z, argb, threads=0) -> "WorldSet":
        """WorldBuilder.SetVoxel per entry, then ToLOD0World + DownSample(1..5)."""
        x = np.ascontiguousarray(x, dtype=np.int32)
        y = np.ascontiguousarray(y, dtype=np.int32)
        z = np.ascontiguousarray(z, dtype=np.int32)
        argb = np.ascontiguousarray(argb, dtype=np.uint32)
        assert x.shape == y.shape == z.shape == argb.shape
        b = C.c_void_p()
        _check(lib().cvxh_world_builder_create(int(dims[0]), int(dims[1]), int(dims[2]), C.byref(b)))
        try:
            _check(lib().cvxh_world_builder_set_voxels(b, x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data, argb.ctypes.data))
            h = C.c_void_p()
            _check(lib().cvxh_world_builder_finish(b, threads, C.byref(h)))
        finally:
            lib().cvxh_world_builder_free(b)
        return WorldSet(h.value)

    @staticmethod
    def from_blobs(dims, blobs) -> "WorldSet":
        """One storage blob (bytes / uint8 array, the reference's layout) per LOD, e.g. LOD 0 from the host build and the
        rest from cpuvox_amd.gpu.Context.downsample."""
        arrays = [np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray)) else np.ascontiguousarray(b, dtype=np.uint8) for b in blobs]
        ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        lens = (C.c_int64 * len(arrays))(*[a.size for a in arrays])
        h = C.c_void_p()
        _check(lib().cvxh_world_from_blobs(int(dims[0]), int(dims[1]), int(dims[2]), len(arrays), ptrs, lens, C.byref(h)))
        return WorldSet(h.value)

    def downsample_host_seconds(self, extra_lods: int, threads: int = 0):
        """Wall-clock seconds (and voxel count) of World.DownSample(extra_lods) of LOD 0 on the host; the result is discarded."""
        sec, vox = C.c_double(), C.c_int64()
        _check(lib().cvxh_world_downsample_seconds(self._h, extra_lods, threads, C.byref(sec), C.byref(vox)))
        return sec.value, vox.value

    # -- accessors --------------------------------------------------------
    def save(self, path: str) -> None:
        """WorldSaveFile.Serialize (WorldSaveFile.cs:8)."""
        _check(lib().cvxh_world_save(self._h, path.encode()))

    @property
    def lod_count(self) -> int:
        return lib().cvxh_world_lod_count(self._h)

    @property
    def lod0_voxels(self) -> int:
        return lib().cvxh_world_lod0_voxels(self._h)

    def info(self, lod: int) -> WorldInfo:
        out = WorldInfo()
        _check(lib().cvxh_world_info_get(self._h, lod, C.byref(out)))
        return out

    @property
    def dims(self):
        i = self.info(0)
        return (i.dimX, i.dimY, i.dimZ)

    @property
    def max_dimension(self) -> int:
        return max(self.dims)

    def storage(self, lod: int) -> np.ndarray:
        """The raw storage blob of one LOD as a uint8 view (no copy)."""
        i = self.info(lod)
        buf = (C.c_uint8 * i.byteLength).from_address(i.storage)
        return np.frombuffer(buf, dtype=np.uint8)

    def extract_region(self, lod: int, x0: int, z0: int, size_x: int, size_z: int):
        """A rectangle of one level (in its own columns) as a sub-world blob for Context.set_columns / Context.edit: (blob bytes,
        column count); column (x, z) is header (x - x0) * size_z + (z - z0)."""
        out, nbytes, columns = C.c_void_p(), C.c_int64(), C.c_int32()
        _check(lib().cvxh_world_extract_region(self._h, lod, x0, z0, size_x, size_z, C.byref(out), C.byref(nbytes), C.byref(columns)))
        try:
            return C.string_at(out.value, nbytes.value), columns.value
        finally:
            lib().cvxh_free(out)

    def close(self) -> None:
        if self._h:
            lib().cvxh_world_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Mesh:
    """A triangle mesh (SimpleMesh, SimpleMesh.cs:11-106) with its materials' diffuse textures, for cpuvox_amd.gpu.Context.stamp_mesh."""

    def __init__(self, handle: int):
        self._h = C.c_void_p(handle)

    @staticmethod
    def from_obj(path: str, swap_yz: bool = False) -> "Mesh":
        """ObjModel.Import (ObjModel.cs:10-171), the file WorldSet.from_obj reads; positions in the model's units until rescale()."""
        h = C.c_void_p()
        _check(lib().cvxh_mesh_load_obj(path.encode(), int(swap_yz), C.byref(h)))
        return Mesh(h.value)

    @staticmethod
    def from_arrays(vertices, indices=None, textures=()) -> "Mesh":
        """A mesh built in code.  vertices: a MESH_VERTEX_DTYPE array, or a dict of arrays {position [N, 3], rgba [N, 4] (default white),
        uv [N, 2] (default 0), material [N] (default -1)}; indices: int32 [3 * T] (default 0 .. N-1); textures: one entry per material,
        None (no texture) or uint8 [H, W, 4] RGBA with row 0 = the bottom row."""
        if isinstance(vertices, dict):
            pos = np.asarray(vertices["position"], dtype=np.float32).reshape(-1, 3)
            v = np.zeros(pos.shape[0], dtype=MESH_VERTEX_DTYPE)
            v["position"] = pos
            v["rgba"] = np.broadcast_to(np.asarray(vertices.get("rgba", 255), dtype=np.uint8), (pos.shape[0], 4))
            v["uv"] = np.broadcast_to(np.asarray(vertices.get("uv", 0.0), dtype=np.float32), (pos.shape[0], 2))
            v["material"] = np.broadcast_to(np.asarray(vertices.get("material", -1), dtype=np.int32), (pos.shape[0],))
        else:
            v = np.ascontiguousarray(np.asarray(vertices).astype(MESH_VERTEX_DTYPE, copy=False))
        idx = np.arange(v.size, dtype=np.int32) if indices is None else np.ascontiguousarray(indices, dtype=np.int32).ravel()
        texels = [None if t is None else np.ascontiguousarray(t, dtype=np.uint8) for t in textures]
        table = (MeshTexture * max(1, len(texels)))()
        for k, t in enumerate(texels):
            if t is not None:
                assert t.ndim == 3 and t.shape[2] == 4, "a texture is uint8 [H, W, 4]"
                table[k].width, table[k].height, table[k].rgba = t.shape[1], t.shape[0], t.ctypes.data
        h = C.c_void_p()
        _check(lib().cvxh_mesh_create(v.ctypes.data if v.size else None, v.size, idx.ctypes.data if idx.size else None, idx.size,
                                      C.cast(table, C.c_void_p), len(texels), C.byref(h)))
        return Mesh(h.value)

    def rescale(self, max_dimension: float, flip=(True, False, False)):
        """SimpleMesh.Rescale (SimpleMesh.cs:49-106) as WorldSet.from_obj applies it (X flipped by default, UnityManager.cs:27): positions in
        LOD-0 voxels of a world of the returned dims (x, y, z)."""
        dims = (C.c_int32 * 3)()
        _check(lib().cvxh_mesh_rescale(self._h, float(max_dimension), int(flip[0]), int(flip[1]), int(flip[2]), dims))
        return tuple(dims)

    @property
    def vertices(self) -> np.ndarray:
        """MESH_VERTEX_DTYPE view of the vertex array (valid until the next rescale / close; rescale changes the positions in place)."""
        p, n = C.c_void_p(), C.c_int32()
        _check(lib().cvxh_mesh_vertices(self._h, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=MESH_VERTEX_DTYPE)
        return np.frombuffer((C.c_uint8 * (n.value * 28)).from_address(p.value), dtype=MESH_VERTEX_DTYPE)

    @property
    def indices(self) -> np.ndarray:
        p, n = C.c_void_p(), C.c_int64()
        _check(lib().cvxh_mesh_indices(self._h, C.byref(p), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, dtype=np.int32)
        return np.frombuffer((C.c_int32 * n.value).from_address(p.value), dtype=np.int32)

    @property
    def material_count(self) -> int:
        return lib().cvxh_mesh_material_count(self._h)

    def texture_struct(self, material: int) -> MeshTexture:
        out = MeshTexture()
        _check(lib().cvxh_mesh_texture(self._h, material, C.byref(out)))
        return out

    def texture(self, material: int):
        """uint8 [H, W, 4] view of material's diffuse texture (row 0 = the bottom row), or None."""
        t = self.texture_struct(material)
        if not t.rgba:
            return None
        return np.frombuffer((C.c_uint8 * (t.width * t.height * 4)).from_address(t.rgba), dtype=np.uint8).reshape(t.height, t.width, 4)

    def close(self) -> None:
        if self._h:
            lib().cvxh_mesh_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_pose(position, euler, width: int, height: int, fov: float = 85.0, near: float = 0.05) -> CameraPose:
    """Scene camera defaults: FOV 85, near 0.05 (Assets/Scenes/SampleScene.unity:176-178)."""
    p = CameraPose()
    p.position[:] = [float(v) for v in position]
    p.eulerAngles[:] = [float(v) for v in euler]
    p.fieldOfView = fov
    p.nearClipPlane = near
    p.pixelWidth = width
    p.pixelHeight = height
    return p


def setup_lods(pose: CameraPose, world_max_dimension: int, res_x: int, res_y: int, lod_error: float = 1.0, repeat: bool = False):
    """UnityManager.SetupLods (UnityManager.cs:417-458) -> (LODDistances[6], farClip).  repeat=True: a repeating world (World.REPEAT_WORLD),
    far clip 10 x world_max_dimension instead of 2 x (UnityManager.cs:421-423)."""
    if not isinstance(repeat, (bool, int)) or int(repeat) not in (0, 1):
        raise ValueError(f"setup_lods: repeat must be a bool, got {repeat!r}")
    out = (C.c_float * LOD_LEVELS)()
    far = C.c_float()
    _check(lib().cvxh_setup_lods_ex(C.byref(pose), world_max_dimension, res_x, res_y, lod_error, int(repeat), out, C.byref(far)))
    return list(out), far.value


def setup_frame(pose: CameraPose, lod_distances, far_clip: float, width: int, height: int, world_dim_y: int, limit_horizon: bool = True) -> Frame:
    """LimitRotationHorizon + the DrawWorld setup before DrawSegments
    (UnityManager.cs:179-181,193-201; RenderManager.cs:119-152)."""
    lods = (C.c_float * LOD_LEVELS)(*lod_distances)
    out = Frame()
    _check(lib().cvxh_setup_frame(C.byref(pose), int(limit_horizon), far_clip, lods, width, height, world_dim_y, C.byref(out)))
    return out


def sample_benchmark_path(t: float, world_dims):
    """BenchmarkPath.anim at clip time t in [0, 1.15] (UnityManager.cs:86-87)."""
    dims = (C.c_float * 3)(*[float(d) for d in world_dims])
    pos = (C.c_float * 3)()
    eul = (C.c_float * 3)()
    lib().cvxh_sample_benchmark_path(t, dims, pos, eul)
    return list(pos), list(eul)


BENCHMARK_PATH_LENGTH = 1.15  # BenchmarkPath.anim:179


def load_image(path: str) -> np.ndarray:
    """Texture2D.LoadImage + GetPixels32 as ObjModel uses them (SimpleMesh.cs:186-205): uint8[H, W, 4] RGBA, row 0 = BOTTOM row."""
    w, h = C.c_int32(), C.c_int32()
    _check(lib().cvxh_image_load(path.encode(), C.byref(w), C.byref(h), None, 0))
    out = np.empty((h.value, w.value, 4), dtype=np.uint8)
    _check(lib().cvxh_image_load(path.encode(), C.byref(w), C.byref(h), out.ctypes.data, out.size))
    return out
