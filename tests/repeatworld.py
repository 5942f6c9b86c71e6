"""Repeating worlds (cvx_set_world_repeat): a world W repeated in X and Z renders exactly like the bounded world T that is W laid out k x k times,
as long as no ray reaches T's edge.  This module builds T from W's blobs and the camera frames the two renders share."""
import numpy as np

from cpuvox_amd import host

# World.RLEColumn (World.cs:161-169): 12 bytes, the element offset counts 4-byte elements from the start of the pool behind the header table
HEADER = np.dtype({"names": ["off", "runs", "lo", "hi"], "formats": ["<i4", "<u2", "<u2", "<u2"], "offsets": [0, 4, 6, 8], "itemsize": 12})


def _table(dx: int, dz: int, lod: int) -> int:
    return (dx * dz) // ((lod + 1) * (lod + 1))  # World.ColumnCount (World.cs:17): the table is longer than the (dx >> lod) x (dz >> lod) columns used


def _split(ws: host.WorldSet, lod: int):
    dx, _, dz = ws.dims
    cx, cz = dx >> lod, dz >> lod
    blob = np.array(ws.storage(lod))
    headers = blob[: cx * cz * 12].view(HEADER).reshape(cx, cz)
    return headers, blob[_table(dx, dz, lod) * 12:]


def tile_blob(ws: host.WorldSet, lod: int, k: int, kz: int | None = None) -> np.ndarray:
    """LOD `lod` of W laid out k x kz times (kz: k where not given): the header table tiled (x-major), every copy of a column pointing at the one
    pool."""
    dx, _, dz = ws.dims
    kz = k if kz is None else kz
    headers, pool = _split(ws, lod)
    table = np.zeros(_table(dx * k, dz * kz, lod), dtype=HEADER)
    tiled = np.tile(headers, (k, kz)).reshape(-1)
    table[: tiled.size] = tiled
    return np.concatenate([table.view(np.uint8), pool])


def tile_world(ws: host.WorldSet, k: int, kz: int | None = None) -> host.WorldSet:
    """W laid out k times along X and kz times along Z (kz: k where not given)."""
    dx, dy, dz = ws.dims
    kz = k if kz is None else kz
    return host.WorldSet.from_blobs((dx * k, dy, dz * kz), [tile_blob(ws, lod, k, kz) for lod in range(host.LOD_LEVELS)])


def column(ws: host.WorldSet, lod: int, x: int, z: int, split=None):
    """(runCount, worldMin, worldMax, elements) of column (x, z) of LOD `lod` (column coordinates): [guard][runs][guard][colours]."""
    headers, pool = split if split is not None else _split(ws, lod)
    h = headers[x, z]
    if h["runs"] == 0:
        return 0, int(h["lo"]), int(h["hi"]), b""
    el = pool.view(np.int16).reshape(-1, 2)
    runs = el[h["off"] + 1: h["off"] + 1 + h["runs"]]
    colours = max([int(c) + int(n) for c, n in runs if c >= 0], default=0)
    return int(h["runs"]), int(h["lo"]), int(h["hi"]), pool[4 * h["off"]: 4 * (h["off"] + h["runs"] + 2 + colours)].tobytes()


def frame(ws_tile: host.WorldSet, width: int, height: int, position, euler, far_clip=None, lod_error: float = 1.0):
    """The frame both renders get: LOD distances of SetupLods in repeat mode for the tile (far clip 10 x its largest dimension), far clip
    replaced by `far_clip` when given."""
    pose = host.camera_pose(position, euler, width, height)
    lods, far = host.setup_lods(pose, ws_tile.max_dimension, width, height, lod_error, repeat=True)
    return host.setup_frame(pose, lods, far if far_clip is None else far_clip, width, height, ws_tile.dims[1], True)
