"""CPU (no GPU needed): the pieces of the in-place world edit that do not need a device.

- The record rule the edit kernels run (cpuvox_amd/csrc/cvx_edit.h), compiled for the host, against the records, counts, run-list blocks and colour
  places cvx_world_upload writes -- on random columns of every shape (one to three derived runs, more runs, air-only, foreign colour indices, bounds
  that disagree with the runs), in a level that keeps colour blocks and one that keeps its colours column after column.
- cvxh_world_extract_region against tests/pyworld.py.
- The three new entry points fail cleanly without a context / device."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import pyworld
import ruleslib
from cpuvox_amd import gpu, host


@pytest.fixture(scope="module")
def rule_binary(tmp_path_factory):
    return ruleslib.build("edit_record_rule", tmp_path_factory.mktemp("rule"))


def _random_column(rng, height, kind, lod):
    """(runs [(colorsIndex, length)], colour count, worldMin, worldMax) of a full-height column in the reference's layout (bounds in LOD-0 voxels)."""
    n = int(rng.integers(1, 9))
    cuts = np.sort(rng.choice(np.arange(1, height), size=min(n - 1, height - 1), replace=False)) if n > 1 else np.array([], dtype=np.int64)
    lengths = np.diff(np.concatenate(([0], cuts, [height]))).tolist()
    solid = rng.random(len(lengths)) < (0.0 if kind == "air" else 0.55)
    if kind != "air" and not solid.any():
        solid[int(rng.integers(0, len(lengths)))] = True
    runs, colours, top = [], 0, height
    spans = []
    for length, s in zip(lengths, solid):
        if s:
            index = colours if kind != "foreign" else int(rng.integers(0, 3))
            runs.append((index, length))
            colours = max(colours, index + length) if kind == "foreign" else colours + length
            spans.append((top - length, top))
        else:
            runs.append((-1, length))
        top -= length
    if spans and kind != "bounds":
        wmin, wmax = spans[-1][0] << lod, spans[0][1] << lod
    else:
        wmin, wmax = int(rng.integers(0, height)), int(rng.integers(0, height + 1))
    return runs, colours, wmin, wmax


def _blob(rng, dims, lod, empty=0.2, deep=None):
    dx, dy, dz = dims
    count = pyworld._column_count(dx, dz, lod)
    ux, uz, height = dx >> lod, dz >> lod, dy >> lod
    headers = bytearray(count * 12)
    elements = bytearray()
    cursor = 0
    for cx in range(ux):
        for cz in range(uz):
            if rng.random() < empty:
                continue
            kind = rng.choice(["derived", "derived", "derived", "air", "foreign", "bounds"])
            runs, colours, wmin, wmax = _random_column(rng, height, kind, lod)
            struct.pack_into("<iHHHH", headers, (cx * uz + cz) * 12, cursor, len(runs), wmin, wmax, 0)
            elements += struct.pack("<hh", 0, 0)
            for index, length in runs:
                elements += struct.pack("<hh", index, length)
            elements += struct.pack("<hh", 0, 0)
            elements += rng.integers(0, 2**32, size=colours, dtype=np.uint64).astype(np.uint32).tobytes()
            cursor += len(runs) + 2 + colours
    return bytes(headers) + bytes(elements), count


@pytest.mark.parametrize("dims,lod,empty,seed", [((64, 64, 64), 0, 0.2, 1), ((64, 128, 32), 1, 0.1, 2), ((128, 64, 64), 2, 0.3, 3),
                                                  ((64, 256, 64), 0, 0.97, 4)])  # the last: a few deep columns -> colours column after column
def test_device_record_rule_matches_the_upload(rule_binary, tmp_path, dims, lod, empty, seed):
    rng = np.random.default_rng(seed)
    blob, count = _blob(rng, dims, lod, empty)
    path = tmp_path / "blob.bin"
    path.write_bytes(blob)
    r = subprocess.run([rule_binary, str(path), *map(str, dims), str(lod), str(count)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout
    words = r.stdout.split()
    columns, listed = int(words[words.index("columns") + 1]), int(words[words.index("listed") + 1])
    assert columns > 0 and listed > 0 and listed < columns, r.stdout


def _py_world(dims, seed):
    rng = np.random.default_rng(seed)
    vox = []
    for _ in range(3000):
        x, y, z = (int(rng.integers(0, d)) for d in dims)
        vox.append((x, y, z, int(rng.integers(0, 2**32))))
    return vox


@pytest.mark.parametrize("lod,rect", [(0, (3, 5, 10, 7)), (0, (0, 0, 32, 32)), (1, (4, 2, 8, 12)), (2, (0, 3, 8, 5))])
def test_extract_region_matches_pyworld(lod, rect):
    dims = (32, 32, 32)
    vox = _py_world(dims, 11 + lod)
    x, y, z, c = (np.array([v[i] for v in vox]) for i in range(4))
    ws = host.WorldSet.from_voxels(dims, x, y, z, c.astype(np.uint32))
    level = pyworld.build_lod0(dims, vox)
    if lod:
        level = pyworld.downsample(level, lod)
    x0, z0, sx, sz = rect
    headers = bytearray(sx * sz * 12)
    elements = bytearray()
    cursor = 0
    for i in range(sx * sz):
        col = level.columns.get((x0 + i // sz, z0 + i % sz))
        if col is None:
            continue
        runs, colours, wmin, wmax = col
        struct.pack_into("<iHHHH", headers, i * 12, cursor, len(runs), wmin, wmax, 0)
        elements += struct.pack("<hh", 0, 0) + b"".join(struct.pack("<hh", a, b) for a, b in runs) + struct.pack("<hh", 0, 0)
        elements += b"".join(struct.pack("<I", v) for v in colours)
        cursor += len(runs) + 2 + len(colours)
    blob, count = ws.extract_region(lod, *rect)
    assert count == sx * sz
    assert blob == bytes(headers) + bytes(elements)


def test_extract_region_rejects_rectangles_outside_the_level():
    ws = host.WorldSet.procedural(64, 64, 64)
    for lod, rect in ((0, (60, 0, 8, 8)), (2, (0, 0, 17, 1)), (0, (-1, 0, 4, 4)), (0, (0, 0, 0, 4)), (6, (0, 0, 1, 1))):
        with pytest.raises(RuntimeError):
            ws.extract_region(lod, *rect)


def test_edit_entry_points_fail_cleanly_without_a_device_or_context():
    L = gpu.lib()
    blob = (C.c_uint8 * 64)()
    assert L.cvx_world_set_columns(None, 0, 0, 0, 1, 1, blob, 64, 1) == -1                          # CVX_ERR_INVALID_ARGUMENT: no context
    assert L.cvx_world_edit(None, 0, 0, 32, 32, blob, 64, 1, 5, None) == -1
    assert L.cvx_world_edit_stats(None, None, None, None) == -1
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_set_columns(h, 0, 0, 0, 1, 1, blob, 64, 1) == -3                       # CVX_ERR_NOT_READY
            assert L.cvx_world_edit(h, 0, 0, 32, 32, blob, 64, 1, 5, None) == -3
            used, abandoned, spare = C.c_int64(), C.c_int64(), C.c_int64()
            assert L.cvx_world_edit_stats(h, C.byref(used), C.byref(abandoned), C.byref(spare)) == 0
            assert (abandoned.value, spare.value) == (0, 0)
        finally:
            L.cvx_destroy(h)
