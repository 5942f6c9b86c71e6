"""CPU (no GPU needed): the rule behind cvx_world_read_region / cvx_world_read_level (cpuvox_amd/csrc/cvx_readback.h), compiled for the host
through tests/readback_rules.cpp.

- The column rule: random builder columns of every level 0..5 (tests/pyworld.py's final_column with voxel scale 2^lod), as records built with
  the edit's record rule (records with 1..3 runs, listed columns of four and more runs, columns as tall as the world) in both colour layouts:
  the rule must give back the column's exact runs, colours and header.
- Foreign columns (split solid runs, split air runs, runs that share colours, a column with no solid run): the same voxels and colours, in
  builder form.
- Whole levels of host-built worlds, laid out by cvx_world_upload on the host and read back as cvx_world_read_level assembles them:
  byte-identical to the uploaded blobs at every level, both colour layouts.
- The new calls without a context / world: bad arguments first, then CVX_ERR_NOT_READY."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import pyworld
import ruleslib
from cpuvox_amd import gpu, host


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("readback_rules", tmp_path_factory.mktemp("readback"))


# ---- the column rule ---------------------------------------------------------------------------------------------------------------------------

def _builder_column(rng, height, lod):
    """A random builder column of a level `height` voxels tall: (final_column result, dense solid, dense colour) or None when empty."""
    solid = np.zeros(height, dtype=bool)
    kind = int(rng.integers(0, 6))
    if kind == 0:  # as tall as the world
        solid[:] = True
    elif kind == 1:  # many runs: a listed column
        solid[::2] = True
        solid[:int(rng.integers(0, height))] = False
    else:
        for _ in range(int(rng.integers(1, 5))):
            lo = int(rng.integers(0, height))
            solid[lo:lo + int(rng.integers(1, max(2, height // 2)))] = True
    ys = np.nonzero(solid)[0][::-1]
    colours = rng.integers(0, 2**32, size=len(ys), dtype=np.uint64).astype(np.uint32)
    col = pyworld.final_column([(int(y), int(c)) for y, c in zip(ys, colours)], height - 1, 1 << lod)
    dense = np.zeros(height, dtype=np.uint32)
    dense[ys] = colours
    return col, solid, dense


def _case(lod, dim_y, stride, base, wmin, wmax, runs, colours):
    words = [lod, dim_y, stride, base, wmin, wmax, len(runs)]
    for ci, n in runs:
        words += [ci, n]
    words += [len(colours)] + [int(c) - (1 << 32) if c >= 1 << 31 else int(c) for c in colours]
    return words


def _run_columns(rules, tmp_path, cases):
    words = [w for c in cases for w in c]
    (tmp_path / "in").write_bytes(np.array(words, dtype=np.int32).tobytes())
    subprocess.check_call([rules, "column", str(tmp_path / "in"), str(tmp_path / "out")])
    out = np.fromfile(tmp_path / "out", dtype=np.uint32)
    at, results = 0, []
    for _ in cases:
        run_count, colours, wmin, wmax = (int(v) for v in out[at:at + 4])
        at += 4
        runs = [(int(r & 0xFFFF) - (0x10000 if r & 0x8000 else 0), int(r >> 16)) for r in out[at:at + run_count]]
        at += run_count
        cols = [int(c) for c in out[at:at + colours]]
        at += colours
        header = [int(h) for h in out[at:at + 3]]
        at += 3
        results.append((runs, cols, wmin, wmax, header))
    assert at == len(out)
    return results


def _expected_header(col):
    if col is None:
        return [0, 0, 0]
    runs, _, wmin, wmax = col
    return [7, len(runs) | (wmin << 16), wmax]


@pytest.mark.parametrize("lod", range(6))
def test_read_column_gives_back_builder_columns(rules, tmp_path, lod):
    rng = np.random.default_rng(100 + lod)
    dim_y = 256
    height = dim_y >> lod
    cases, want = [], []
    for i in range(400):
        col, _, _ = _builder_column(rng, height, lod)
        if col is None:
            continue
        runs, colours, wmin, wmax = col
        stride = 32 if i % 2 else 1
        base = int(rng.integers(32, 1000))
        cases.append(_case(lod, dim_y, stride, base, wmin, wmax, runs, colours))
        want.append(col)
    got = _run_columns(rules, tmp_path, cases)
    listed = sum(1 for col in want if sum(1 for ci, _ in col[0] if ci >= 0) > 3)
    assert listed > 5, "the cases must include listed columns"
    assert any(col[3] == (dim_y & 0xFFFF) and col[2] == 0 for col in want), "and a column as tall as the world"
    for k, (col, (runs, cols, wmin, wmax, header)) in enumerate(zip(want, got)):
        assert runs == list(col[0]), (k, runs, col[0])
        assert cols == [int(c) for c in col[1]], k
        assert (wmin, wmax) == (col[2], col[3]), k
        assert header == _expected_header(col), k


def _foreign(rng, col, kind):
    """A column with the same voxels in another encoding."""
    runs, colours, _, _ = col
    runs = list(runs)
    if kind == "split-solid":
        k = next((i for i, (ci, n) in enumerate(runs) if ci >= 0 and n >= 2), None)
        if k is None:
            return None
        ci, n = runs[k]
        cut = int(rng.integers(1, n))
        runs[k:k + 1] = [(ci, cut), (ci + cut, n - cut)]
        return runs, list(colours)
    if kind == "split-air":
        k = next((i for i, (ci, n) in enumerate(runs) if ci < 0 and n >= 2), None)
        if k is None:
            return None
        _, n = runs[k]
        cut = int(rng.integers(1, n))
        runs[k:k + 1] = [(-1, cut), (-1, n - cut)]
        return runs, list(colours)
    # shared: every solid run keeps its colours at the front of its own copy, runs in reverse order of the pool
    solid = [(i, ci, n) for i, (ci, n) in enumerate(runs) if ci >= 0]
    pool, out = [], list(runs)
    for i, ci, n in reversed(solid):
        out[i] = (len(pool), n)
        pool += [colours[ci + j] for j in range(n)]
    return out, pool


def _dense_of(runs, colours, height):
    solid = np.zeros(height, dtype=bool)
    dense = np.zeros(height, dtype=np.uint32)
    top = height
    for ci, n in runs:
        if ci >= 0:
            for j in range(n):
                solid[top - 1 - j] = True
                dense[top - 1 - j] = colours[ci + j]
        top -= n
    return solid, dense


@pytest.mark.parametrize("lod", [0, 2, 5])
def test_read_column_turns_foreign_columns_into_builder_form(rules, tmp_path, lod):
    rng = np.random.default_rng(200 + lod)
    dim_y = 512
    height = dim_y >> lod
    cases, want = [], []
    for i in range(300):
        col, solid, dense = _builder_column(rng, height, lod)
        if col is None:
            continue
        f = _foreign(rng, col, ["split-solid", "split-air", "shared"][i % 3])
        if f is None:
            continue
        runs, colours = f
        s2, d2 = _dense_of(runs, colours, height)
        assert (s2 == solid).all() and (d2 == dense).all()
        cases.append(_case(lod, dim_y, 32 if i % 2 else 1, int(rng.integers(32, 500)), 0, 0, runs, colours))
        want.append(col)
    # a column of air runs only: no solid voxel, read back as the empty column
    cases.append(_case(lod, dim_y, 1, 40, 0, 0, [(-1, height // 2), (-1, height - height // 2)], []))
    want.append(None)
    got = _run_columns(rules, tmp_path, cases)
    assert len(cases) > 150
    for k, (col, (runs, cols, wmin, wmax, header)) in enumerate(zip(want, got)):
        if col is None:
            assert (runs, cols, header) == ([], [], [0, 0, 0]), k
            continue
        assert runs == list(col[0]), (k, runs, col[0])
        assert cols == [int(c) for c in col[1]], k
        assert (wmin, wmax) == (col[2], col[3]), k
        assert header == _expected_header(col), k


# ---- whole levels ------------------------------------------------------------------------------------------------------------------------------

def _terrain_world(dims, seed):
    rng = np.random.default_rng(seed)
    dx, dy, dz = dims
    x, y, z = np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij")
    h = dy // 4 + (dy // 8 * np.sin(x / 5.0) + dy // 10 * np.cos(z / 4.0)).astype(np.int64)
    solid = y < h
    solid |= (y >= dy // 2) & (y < dy // 2 + 3) & ((x // 8 + z // 8) % 3 == 0)
    solid |= (y % 4 == 0) & (x % 7 == 3) & (z % 5 == 1)  # many-run columns
    solid &= rng.random(solid.shape) > 0.02
    return solid


def _sparse_world(dims, seed):
    rng = np.random.default_rng(seed)
    solid = np.zeros(dims, dtype=bool)
    for _ in range(60):
        x, z = rng.integers(0, dims[0]), rng.integers(0, dims[2])
        lo = int(rng.integers(0, dims[1] // 3))
        solid[x, lo:lo + int(rng.integers(dims[1] // 4, dims[1] // 2)), z] = True
    return solid


@pytest.mark.parametrize("kind", ["terrain", "sparse"])
def test_read_level_is_byte_identical_for_host_built_worlds(rules, tmp_path, kind):
    dims = (64, 64, 64) if kind == "terrain" else (64, 256, 64)
    solid = _terrain_world(dims, 3) if kind == "terrain" else _sparse_world(dims, 4)
    x, y, z = np.nonzero(solid)
    argb = (0xFF000000 | ((x * 2654435761 + y * 40503 + z * 2246822519) >> 5 & 0xFFFFFF)).astype(np.uint32)
    ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), argb, threads=2)
    shifts = set()
    try:
        for lod in range(6):
            info = ws.info(lod)
            blob = ws.storage(lod).tobytes()
            (tmp_path / "blob").write_bytes(blob)
            out = subprocess.check_output([rules, "level", str(tmp_path / "blob"), str(lod), str(dims[0]), str(dims[1]), str(dims[2]),
                                           str(info.columnCount), str(tmp_path / "out")], text=True)
            shifts.add(out.split()[1])
            got = (tmp_path / "out").read_bytes()
            assert info.columnCount == pyworld._column_count(dims[0], dims[2], lod)
            assert got == blob, f"LOD {lod}: {len(got)} bytes against {len(blob)}"
    finally:
        ws.close()
    assert shifts == {"7"} if kind == "terrain" else "2" in shifts, shifts  # (the sparse world keeps its colours column after column)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------

def test_new_calls_fail_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    out, nbytes, columns = C.c_void_p(), C.c_int64(), C.c_int32()
    reclaimed, ms = C.c_int64(), C.c_float()
    assert L.cvx_world_read_region(None, 0, 0, 0, 1, 1, C.byref(out), C.byref(nbytes), C.byref(columns)) == -1  # CVX_ERR_INVALID_ARGUMENT
    assert L.cvx_world_read_level(None, 0, C.byref(out), C.byref(nbytes), C.byref(columns)) == -1
    assert L.cvx_world_compact(None, C.byref(reclaimed), C.byref(ms)) == -1
    # a context without a device or world (tests/readback_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 9 + [-3] * 3, codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_read_level(h, 0, C.byref(out), C.byref(nbytes), C.byref(columns)) == -3
            assert L.cvx_world_compact(h, C.byref(reclaimed), C.byref(ms)) == -3
        finally:
            L.cvx_destroy(h)


def test_python_wrappers_exist():
    for name in ("read_region", "read_level", "download", "compact"):
        assert callable(getattr(gpu.Context, name)), name
    with pytest.raises(gpu.CvxError):
        gpu.Context.download(type("NoWorld", (), {"dims": None})())
