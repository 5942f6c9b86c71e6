"""CPU (no GPU needed): the rules behind cvx_world_brush and cvx_world_pick (cpuvox_amd/csrc/cvx_brush.h), compiled for the host through
tests/brush_rules.cpp, against independent numpy models.

- The brush column rule: thousands of random columns (0..8 runs; records with 1..3 runs and listed columns; blocked and column-after-column
  colour layouts at arbitrary places) and random stroke lists, against a dense per-column model re-encoded with tests/pyworld.py's
  final_column: runs, colours, worldMin / worldMax and the over-limit rejections must match exactly.
- The pick walk: random rays through small random worlds uploaded into a host-only context, against the float64 dense 3-D DDA of
  tests/pickmodel.py; exact on every ray the model calls unambiguous, and at least 99 % of the rays are.
- The new calls without a context / world (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pickmodel
import pyworld
import ruleslib
from cpuvox_amd import gpu, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("brush_rules", tmp_path_factory.mktemp("brush"))


# ---- the brush column rule ---------------------------------------------------------------------------------------------------------------------

def _stroke(op, shape, a, b, argb=0):
    return {"op": op, "shape": shape, "a": list(a), "b": list(b), "argb": argb & 0xFFFFFFFF}


def _random_column(rng, dim_y):
    """(runs [(colorsIndex, length)], colours) of a full-height column of up to 8 runs, and the dense (solid, colour) it stands for."""
    kind = rng.choice(["builder", "builder", "split", "shared"])
    solid = np.zeros(dim_y, dtype=bool)
    spans = int(rng.integers(0, 5))
    for _ in range(spans):
        lo = int(rng.integers(0, dim_y))
        solid[lo:lo + int(rng.integers(1, max(2, dim_y // 3)))] = True
    ys = np.nonzero(solid)[0][::-1]
    cols = rng.integers(0, 2**32, size=len(ys), dtype=np.uint64).astype(np.uint32)
    col = pyworld.final_column([(int(y), int(c)) for y, c in zip(ys, cols)], dim_y - 1, 1)
    if col is None:
        return [], [], solid, np.zeros(dim_y, dtype=np.uint32)
    runs, colours, _, _ = col
    runs = list(runs)
    if kind == "split":  # a solid run cut into two adjacent ones (still derived indices, no longer maximal runs)
        k = next((i for i, (ci, n) in enumerate(runs) if ci >= 0 and n >= 2), None)
        if k is not None:
            ci, n = runs[k]
            cut = int(rng.integers(1, n))
            runs[k:k + 1] = [(ci, cut), (ci + cut, n - cut)]
    if kind == "shared":  # colour indices that are not the running sum (a listed column): every run starts at colour 0
        runs = [(0 if ci >= 0 else ci, n) for ci, n in runs]
        longest = max(n for ci, n in runs if ci >= 0)
        colours = colours[:longest]
    dense = np.zeros(dim_y, dtype=np.uint32)
    top = dim_y
    for ci, n in runs:
        if ci >= 0:
            for i in range(n):
                dense[top - 1 - i] = colours[ci + i]
        top -= n
    return runs, list(colours), solid, dense


def _random_strokes(rng, cx, cz, dim_y):
    out = []
    for _ in range(int(rng.integers(0, 7))):
        op, shape = int(rng.integers(0, 3)), int(rng.integers(0, 2))
        argb = int(rng.integers(0, 2**32))
        if shape == 0:
            a = [cx - int(rng.integers(-1, 3)), int(rng.integers(-4, dim_y)), cz - int(rng.integers(-1, 3))]
            b = [a[0] + int(rng.integers(0, 4)), a[1] + int(rng.integers(0, dim_y // 2 + 2)), a[2] + int(rng.integers(0, 4))]
        else:
            r = int(rng.integers(0, dim_y // 3 + 2))
            a = [cx + int(rng.integers(-r - 1, r + 2)), int(rng.integers(-r, dim_y + r)), cz + int(rng.integers(-r - 1, r + 2))]
            b = [r, int(rng.integers(-5, 5)), int(rng.integers(-5, 5))]  # (b[1..2] of a sphere are ignored)
        out.append(_stroke(op, shape, a, b, argb))
    return out


def _model_column(solid, dense, strokes, cx, cz, dim_y):
    """The column after the strokes, re-encoded by the builder's rule: (over_limit, runs words, colours, worldMin, worldMax)."""
    s = solid.reshape(1, dim_y, 1).copy()
    c = dense.reshape(1, dim_y, 1).copy()
    shifted = [dict(st, a=[st["a"][0] - cx, st["a"][1], st["a"][2] - cz],
                    b=[st["b"][0] - cx, st["b"][1], st["b"][2] - cz] if st["shape"] == 0 else st["b"]) for st in strokes]
    pickmodel.apply_strokes(s, c, shifted)
    ys = np.nonzero(s[0, :, 0])[0][::-1]
    col = pyworld.final_column([(int(y), int(c[0, y, 0])) for y in ys], dim_y - 1, 1)
    if col is None:
        return False, [], [], 0, 0
    runs, colours, wmin, wmax = col
    over = len(runs) > 65535 or any(n > 32767 for _, n in runs) or any(ci > 32767 for ci, _ in runs)
    words = [((ci & 0xFFFF) | (n << 16)) for ci, n in runs]
    return over, words, colours, wmin, wmax


def _case_words(dim_y, cx, cz, stride, base, runs, colours, strokes):
    w = [dim_y, cx, cz, stride] + ruleslib.column_words(base, runs, colours) + [len(strokes)]
    for s in strokes:
        w += [s["op"], s["shape"], *s["a"], *s["b"], int(np.int32(np.uint32(s["argb"]))), 0]
    return w


def _run_brush(rules, tmp_path, cases):
    words = []
    for case in cases:
        words += _case_words(*case)
    out = ruleslib.run_cases(rules, "brush", tmp_path, words)
    results, at = ruleslib.edited_columns(out, 0, len(cases))
    assert at == len(out)
    return results


def test_brush_column_rule_matches_the_dense_model(rules, tmp_path):
    rng = np.random.default_rng(2026)
    cases, models = [], []
    for i in range(3000):
        dim_y = int(rng.choice([8, 16, 64, 256]))
        cx, cz = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        runs, colours, solid, dense = _random_column(rng, dim_y)
        strokes = _random_strokes(rng, cx, cz, dim_y)
        stride = int(rng.choice([1, 32]))
        base = int(rng.integers(32, 5000))
        cases.append((dim_y, cx, cz, stride, base, runs, colours, strokes))
        models.append(_model_column(solid, dense, strokes, cx, cz, dim_y))
    results = _run_brush(rules, tmp_path, cases)
    bad = [i for i, (got, want) in enumerate(zip(results, models)) if got[0] != want[0] or (not got[0] and list(got[1:]) != list(want[1:]))]
    assert not bad, f"{len(bad)} of {len(cases)} columns differ; first {bad[0]}: case {cases[bad[0]]}\n got {results[bad[0]]}\nwant {models[bad[0]]}"
    touched = sum(1 for c in cases if c[7])
    assert touched > 2000 and sum(1 for c in cases if len(c[5]) > 3) > 100


def test_brush_column_rule_rejects_what_the_format_cannot_hold(rules, tmp_path):
    """A run longer than 32767 voxels and a colour index above 32767 (World.cs:161-259 keeps them in shorts) are over the limit; columns just
    inside the limits are not."""
    H = 65536
    cases = [
        (H, 0, 0, 1, 32, [], [], [_stroke(0, 0, (0, 0, 0), (1, 32768, 1), 5)]),                                 # one run of 32768
        (H, 0, 0, 1, 32, [], [], [_stroke(0, 0, (0, 1, 0), (1, 32768, 1), 5)]),                                 # 32767 solid + air 32768 above
        (H, 0, 0, 1, 32, [], [], [_stroke(0, 0, (0, 45000, 0), (1, 65536, 1), 5), _stroke(0, 0, (0, 30000, 0), (1, 44999, 1), 6),
                                  _stroke(0, 0, (0, 1, 0), (1, 29999, 1), 7)]),                                   # third run's index 35535
        (16384, 0, 0, 32, 32, [], [], [_stroke(0, 0, (0, 0, 0), (1, 16384, 1), 5)]),                           # one run of 16384: fine
        (16384, 0, 0, 32, 32, [], [], [_stroke(0, 0, (0, 0, 0), (1, 16384, 1), 5), _stroke(1, 0, (0, 100, 0), (1, 101, 1))]),
    ]
    results = _run_brush(rules, tmp_path, cases)
    assert [r[0] for r in results] == [True, True, True, False, False]
    assert results[3][1] == [0 | (16384 << 16)] and results[3][3:] == (0, 16384)
    assert len(results[4][1]) == 3 and results[4][1][2] == (16283 | (100 << 16))


# ---- the pick walk -----------------------------------------------------------------------------------------------------------------------------

def _pick_world(rng, dims, sparse=False):
    dx, dy, dz = dims
    x, y, z = np.meshgrid(np.arange(dx), np.arange(dy), np.arange(dz), indexing="ij")
    if sparse:  # deep columns far apart: blocks would waste more than 4 x, the colours are kept column after column
        solid = np.zeros(dims, dtype=bool)
        for _ in range(100):
            cx, cz = rng.integers(0, dx), rng.integers(0, dz)
            lo = int(rng.integers(0, 50))
            solid[cx, lo:lo + int(rng.integers(50, 200)), cz] = True
    else:
        h = dy // 4 + (3 * np.sin(x / 3.0) + 2 * np.cos(z / 4.0)).astype(np.int64)
        solid = y < h
        solid |= (y >= dy // 2) & (y < dy // 2 + 2) & ((x // 4 + z // 4) % 3 == 0)           # floating slabs
        solid |= (x % 7 == 3) & (z % 5 == 1) & (y % 3 == 0)                                   # columns of many runs
        solid &= ~((x - dx // 2) ** 2 + (z - dz // 2) ** 2 + (y - dy // 4) ** 2 < 16)          # a crater
    xs, ys, zs = np.nonzero(solid)
    colour = np.zeros(dims, dtype=np.uint32)
    colour[xs, ys, zs] = (0xFF000000 | ((xs * 2654435761 + ys * 40503 + zs * 2246822519) >> 7) & 0xFFFFFF).astype(np.uint32)
    ws = host.WorldSet.from_voxels(dims, xs.astype(np.int32), ys.astype(np.int32), zs.astype(np.int32), colour[xs, ys, zs], threads=2)
    return solid, colour, ws


def _run_pick(rules, tmp_path, ws, origins, directions, max_t):
    info = ws.info(0)
    blob, rays_in, hits_out = tmp_path / "world.bin", tmp_path / "rays.bin", tmp_path / "hits.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    rays = np.zeros(len(origins), dtype=gpu.PICK_RAY_DTYPE)
    rays["origin"], rays["direction"], rays["maxT"] = origins, directions, max_t
    rays_in.write_bytes(rays.tobytes())
    text = subprocess.check_output([rules, "pick", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(rays_in), str(hits_out)],
                                   text=True)
    hits = np.frombuffer(hits_out.read_bytes(), dtype=gpu.PICK_HIT_DTYPE)
    m = re.match(r"colorShift (\d+) listed (\d+)", text)
    return hits, int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("dims,sparse,seed", [((32, 32, 32), False, 1), ((16, 64, 32), False, 2), ((64, 256, 64), True, 3)])
def test_pick_walk_matches_the_float64_model(rules, tmp_path, dims, sparse, seed):
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    try:
        o, d, max_t = pickmodel.random_rays(rng, dims, 3000)
        hits, colour_shift, listed = _run_pick(rules, tmp_path, ws, o, d, max_t)
    finally:
        ws.close()
    assert colour_shift == (2 if sparse else 7)
    if not sparse:
        assert listed > 0, "the world must have listed columns"
    model = pickmodel.pick_many(solid, colour, o, d, max_t)
    fraction = pickmodel.compare_picks(hits, model, f"{dims}")
    assert fraction >= 0.99, f"only {fraction:.4f} of the rays are unambiguous"
    faces = model[1]
    assert (faces == -1).sum() > 100 and (faces == 6).sum() > 20 and all((faces == f).sum() > (0 if sparse else 5) for f in range(6)), np.bincount(faces + 1)


# ---- layouts and entry points ------------------------------------------------------------------------------------------------------------------

def test_new_calls_fail_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    stroke = gpu.strokes_array([_stroke(0, 0, (0, 0, 0), (1, 1, 1))])
    ms = C.c_float()
    assert L.cvx_world_brush(None, stroke.ctypes.data, 1, 0, C.byref(ms)) == -1                      # CVX_ERR_INVALID_ARGUMENT: no context
    rays = np.zeros(1, dtype=gpu.PICK_RAY_DTYPE)
    hits = np.zeros(1, dtype=gpu.PICK_HIT_DTYPE)
    assert L.cvx_world_pick(None, 1, rays.ctypes.data, hits.ctypes.data) == -1
    assert L.cvx_world_pick_device(None, 1, None, None, None) == -1
    # a context without a device or world (tests/brush_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 8 + [-3] + [-1, -1, -3, -1], codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_brush(h, stroke.ctypes.data, 1, 0, C.byref(ms)) == -3
            assert L.cvx_world_pick(h, 1, rays.ctypes.data, hits.ctypes.data) == -3
        finally:
            L.cvx_destroy(h)


def test_strokes_array_accepts_dicts_and_structured_arrays():
    a = gpu.strokes_array([{"op": gpu.BRUSH_CARVE, "shape": gpu.SHAPE_SPHERE, "a": (3, 4, 5), "radius": 7},
                           {"op": gpu.BRUSH_FILL, "shape": gpu.SHAPE_BOX, "a": (0, 0, 0), "b": (2, 3, 4), "argb": 0xFF112233}])
    assert a["b"].tolist() == [[7, 0, 0], [2, 3, 4]] and a["argb"].tolist() == [0, 0xFF112233]
    assert gpu.strokes_array(a) is a or (gpu.strokes_array(a) == a).all()
    raw = a.tobytes()
    assert struct.unpack_from("<iiiiiiiiIi", raw, 40) == (0, 0, 0, 0, 0, 2, 3, 4, 0xFF112233, 0)
