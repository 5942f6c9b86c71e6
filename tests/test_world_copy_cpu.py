"""CPU (no GPU needed): the column rule behind cvx_world_copy (cpuvox_amd/csrc/cvx_copy.h), compiled for the host through tests/copy_rules.cpp,
against the independent dense model of tests/copymodel.py.

- Column mode: thousands of random columns in small worlds (records with 1..3 runs and listed columns, blocked and column-after-column colour
  layouts, foreign encodings) under random placement lists, against the dense model re-encoded with tests/pyworld.py's final_column: runs,
  colours, worldMin / worldMax and the over-limit rejections must match exactly.
- World mode: small random worlds uploaded into a host-only context; the rule over every column of the call's rectangle gives the sub-world blob
  the write kernel makes, which must equal, byte for byte, the same rectangle of the model's world built on the host.  All 16 transforms, the four
  ops, moves onto themselves, later placements over earlier ones, destinations partly and wholly outside the world.
- The call without a context / world; copy_placements_array (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import copymodel
import pyworld
import ruleslib
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world, _random_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, CARVE, PAINT, REPLACE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT, gpu.COPY_REPLACE


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("copy_rules", tmp_path_factory.mktemp("copy"))


def _placement(src_min, src_max, dst, transform=0, op=REPLACE, move=0):
    return {"srcMin": list(src_min), "srcMax": list(src_max), "dst": list(dst), "transform": transform, "op": op, "move": move}


def rectangle(placements, dims, level_count):
    """cvx_world_copy's rectangle (x0, z0, sizeX, sizeZ), or None when nothing changes."""
    x0 = z0 = 1 << 40
    x1 = z1 = -(1 << 40)
    for p in gpu.copy_placements_array(placements):
        a, b, d = [int(v) for v in p["srcMin"]], [int(v) for v in p["srcMax"]], [int(v) for v in p["dst"]]
        size = [b[0] - a[0], b[1] - a[1], b[2] - a[2]]
        if int(p["transform"]) & 1:
            size[0], size[2] = size[2], size[0]
        lo = [max(d[i], 0) for i in range(3)]
        hi = [min(d[i] + size[i], dims[i]) for i in range(3)]
        if all(lo[i] < hi[i] for i in range(3)):
            x0, x1, z0, z1 = min(x0, lo[0]), max(x1, hi[0]), min(z0, lo[2]), max(z1, hi[2])
        if int(p["move"]):
            x0, x1, z0, z1 = min(x0, a[0]), max(x1, b[0]), min(z0, a[2]), max(z1, b[2])
    if x1 < x0:
        return None
    m = (1 << level_count) - 1
    x0, z0 = x0 & ~m, z0 & ~m
    x1, z1 = min((x1 + m) & ~m, dims[0]), min((z1 + m) & ~m, dims[2])
    return x0, z0, x1 - x0, z1 - z0


# ---- column mode -------------------------------------------------------------------------------------------------------------------------------

def _random_placements(rng, gx, dim_y, gz):
    out = []
    for _ in range(int(rng.integers(0, 5))):
        a, b = [], []
        for dim in (gx, dim_y, gz):
            lo = int(rng.integers(0, dim))
            a.append(lo)
            b.append(int(rng.integers(lo + 1, dim + 1)))
        size = [b[i] - a[i] for i in range(3)]
        dst = [int(rng.integers(-size[0], gx + 1)), int(rng.integers(-size[1] - 2, dim_y + 2)), int(rng.integers(-size[2], gz + 1))]
        out.append(_placement(a, b, dst, int(rng.integers(0, 16)), int(rng.integers(0, 4)), int(rng.random() < 0.3)))
    return out


def _model_columns(solid, colour, placements):
    """Per column (x-major): (over_limit, runs words, colours, worldMin, worldMax) of the model's result re-encoded by the builder's rule."""
    s, c = copymodel.apply_copies(solid, colour, gpu.copy_placements_array(placements))
    gx, dim_y, gz = solid.shape
    out = []
    for x in range(gx):
        for z in range(gz):
            ys = np.nonzero(s[x, :, z])[0][::-1]
            col = pyworld.final_column([(int(y), int(c[x, y, z])) for y in ys], dim_y - 1, 1)
            if col is None:
                out.append((False, [], [], 0, 0))
                continue
            runs, colours, wmin, wmax = col
            over = len(runs) > 65535 or any(n > 32767 for _, n in runs) or any(ci > 32767 for ci, _ in runs)
            out.append((over, [((ci & 0xFFFF) | (n << 16)) for ci, n in runs], list(colours), wmin, wmax))
    return out


def _run_columns(rules, tmp_path, cases):
    """cases: (dim_y, gx, gz, stride, [(colorsBase, runs, colours)] x-major, placements) -> per case, per column (over, runs, colours, wmin, wmax)."""
    words = []
    for dim_y, gx, gz, stride, columns, placements in cases:
        arr = gpu.copy_placements_array(placements)
        words += ruleslib.world_words(dim_y, gx, gz, stride, columns) + [len(arr)] + np.frombuffer(arr.tobytes(), dtype=np.int32).tolist()
    out = ruleslib.run_cases(rules, "columns", tmp_path, words)
    results, at = [], 0
    for dim_y, gx, gz, *_ in cases:
        per, at = ruleslib.edited_columns(out, at, gx * gz)
        results.append(per)
    assert at == len(out)
    return results


def _compare(results, models, cases):
    bad = [(i, k) for i, (got, want) in enumerate(zip(results, models)) for k, (g, w) in enumerate(zip(got, want))
           if g[0] != w[0] or (not g[0] and list(g[1:]) != list(w[1:]))]
    if bad:
        i, k = bad[0]
        raise AssertionError(f"{len(bad)} columns differ; first: case {i} column {k}: {cases[i]}\n got {results[i][k]}\nwant {models[i][k]}")


def test_copy_column_rule_matches_the_dense_model(rules, tmp_path):
    rng = np.random.default_rng(2027)
    cases, models = [], []
    columns_total = listed_like = covered = 0
    for _ in range(1200):
        dim_y = int(rng.choice([8, 16, 64, 256]))
        gx, gz = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        stride = int(rng.choice([1, 32]))
        solid = np.zeros((gx, dim_y, gz), dtype=bool)
        colour = np.zeros((gx, dim_y, gz), dtype=np.uint32)
        columns = []
        for k in range(gx * gz):
            runs, colours, _, dense = _random_column(rng, dim_y)
            x, z = k // gz, k % gz
            for y in range(dim_y):  # the column's voxels as its runs say (a "split" / "shared" column included)
                colour[x, y, z] = dense[y]
            top = dim_y
            for ci, n in runs:
                if ci >= 0:
                    solid[x, top - n:top, z] = True
                top -= n
            base = 32 + k * 20000 + int(rng.integers(0, 100))
            columns.append((base, runs, colours))
            listed_like += sum(1 for ci, _ in runs if ci >= 0) > 3
        colour[~solid] = 0
        placements = _random_placements(rng, gx, dim_y, gz)
        cases.append((dim_y, gx, gz, stride, columns, placements))
        models.append(_model_columns(solid, colour, placements))
        columns_total += gx * gz
        covered += bool(placements)
    results = _run_columns(rules, tmp_path, cases)
    _compare(results, models, cases)
    assert columns_total > 5000 and listed_like > 200 and covered > 900, (columns_total, listed_like, covered)


def test_copy_column_rule_rejects_what_the_format_cannot_hold(rules, tmp_path):
    """A run longer than 32767 voxels and a colour index above 32767 (World.cs:161-259 keeps them in shorts) are over the limit, whether the
    copy makes them from one source or from several; columns just inside the limits are not."""
    H = 50000

    def column(*spans):  # solid spans [lo, hi) -> (runs, colours), the builder's encoding
        s = np.zeros(H, dtype=bool)
        for lo, hi in spans:
            s[lo:hi] = True
        ys = np.nonzero(s)[0][::-1]
        runs, colours, _, _ = pyworld.final_column([(int(y), 0xFF000000 | int(y)) for y in ys], H - 1, 1)
        return s, runs, colours

    specs = [
        # (column 0 spans, column 1 spans, placements onto column 0) in a 2 x 1 world
        ([(0, 20000)], [(20000, 40000)], [_placement((1, 20000, 0), (2, 40000, 1), (0, 20000, 0), op=FILL)]),          # one run of 40000
        ([(0, 17000)], [(17001, 34001), (34002, 50000)], [_placement((1, 17001, 0), (2, 50000, 1), (0, 17001, 0))]),   # third index 32998
        ([(0, 16000)], [(16000, 32767)], [_placement((1, 16000, 0), (2, 32767, 1), (0, 16000, 0), op=FILL)]),          # 32767: fine
        ([(0, 20000)], [(20000, 40000)], [_placement((1, 20000, 0), (2, 40000, 1), (0, 20000, 0), transform=8, op=FILL),
                                          _placement((0, 10000, 0), (1, 10001, 1), (0, 10000, 0), op=CARVE, move=1)]),  # cut in two: fine
    ]
    cases, models = [], []
    for c0, c1, placements in specs:
        s0, r0, k0 = column(*c0)
        s1, r1, k1 = column(*c1)
        solid = np.stack([s0, s1])[:, :, None]
        colour = np.where(solid, (0xFF000000 | np.arange(H, dtype=np.uint32))[None, :, None], 0).astype(np.uint32)
        cases.append((H, 2, 1, 1, [(32, r0, k0), (32 + 60000, r1, k1)], placements))
        models.append(_model_columns(solid, colour, placements))
    results = _run_columns(rules, tmp_path, cases)
    assert [r[0][0] for r in results] == [True, True, False, False]
    assert [m[0][0] for m in models] == [True, True, False, False]
    _compare(results, models, cases)


# ---- world mode ---------------------------------------------------------------------------------------------------------------------------------

def _run_world(rules, tmp_path, ws, placements, rect):
    info = ws.info(0)
    blob, pl, out = tmp_path / "world.bin", tmp_path / "placements.bin", tmp_path / "sub.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    pl.write_bytes(gpu.copy_placements_array(placements).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount), str(pl),
                                    *[str(v) for v in rect], str(out)], text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) over (\d+)", text)
    return out.read_bytes(), int(m.group(1)), int(m.group(2)), int(m.group(3))


def world_cases(dims):
    """Named placement lists over a world of `dims` (the GPU test uses them too)."""
    dx, dy, dz = dims
    box = ((4, 2, 6), (14, dy // 2, 13))  # 10 x (dy/2 - 2) x 7
    cases = {}
    for t in range(16):
        cases[f"transform {t}"] = [_placement(*box, (dx // 2 - 3, dy // 4, dz // 2 - 5), t)]
    for name, op in (("fill", FILL), ("carve", CARVE), ("paint", PAINT), ("replace", REPLACE)):
        cases[name] = [_placement(*box, (dx // 2, 1, dz // 3), 5, op)]
    cases["overlapping move"] = [_placement((3, 0, 3), (dx // 2 + 3, dy, dz // 2 + 1), (7, 3, 6), 0, REPLACE, 1)]
    cases["overlapping move turned"] = [_placement((2, 1, 4), (dx // 2, dy - 4, dz // 2 + 6), (5, 2, 3), 3, FILL, 1)]
    cases["later over earlier"] = [_placement(*box, (dx // 2, 3, dz // 2), 0, REPLACE),
                                   _placement((0, 0, 0), (6, dy, 6), (dx // 2 + 2, 0, dz // 2 + 2), 2, CARVE),
                                   _placement((1, 3, 1), (9, dy - 2, 9), (dx // 2 + 4, 1, dz // 2 + 1), 9, PAINT),
                                   _placement(*box, (dx // 2 + 1, 3, dz // 2 - 2), 14, FILL, 1)]
    cases["partly outside"] = [_placement(*box, (dx - 5, dy - 6, -3), 7), _placement(*box, (-4, -3, dz - 4), 1, FILL)]
    cases["wholly outside, moving"] = [_placement(*box, (dx + 2, 0, 0), 0, REPLACE, 1), _placement(*box, (0, dy, 0), 0, FILL)]
    cases["wholly outside"] = [_placement(*box, (-40, 0, 0), 0, REPLACE)]
    return cases


def snapshot_matters(solid, colour, placements):
    """Whether a rule that reads the half-written result (the moves' carves and the placements before it) instead of the snapshot gives another
    world: a case for which it does tells the two apart."""
    arr = gpu.copy_placements_array(placements)
    s, c = copymodel.apply_copies(solid, colour, [dict(srcMin=p["srcMin"], srcMax=p["srcMax"], dst=(1 << 30, 0, 0), transform=0, op=FILL, move=p["move"])
                                                  for p in arr])
    for p in arr.copy():
        p["move"] = 0
        s, c = copymodel.apply_copies(s, c, [p])
    want = copymodel.apply_copies(solid, colour, arr)
    return not ((s == want[0]).all() and (c == want[1]).all())


@pytest.mark.parametrize("dims,sparse,level_count,seed", [((32, 32, 32), False, 3, 1), ((16, 64, 32), False, 0, 2), ((32, 128, 32), True, 5, 3)])
def test_copied_rectangle_equals_the_model_world(rules, tmp_path, dims, sparse, level_count, seed):
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    checked = 0
    try:
        for name, placements in world_cases(dims).items():
            rect = rectangle(placements, dims, level_count)
            if name == "wholly outside":
                assert rect is None
                continue
            if name.startswith("overlapping"):
                assert snapshot_matters(solid, colour, placements), f"{name}: does not tell the snapshot from the half-written result"
            s, c = copymodel.apply_copies(solid, colour, gpu.copy_placements_array(placements))
            x, y, z = np.nonzero(s)
            want_ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), c[x, y, z], threads=2)
            try:
                want, _ = want_ws.extract_region(0, *rect)
            finally:
                want_ws.close()
            got, colour_shift, listed, over = _run_world(rules, tmp_path, ws, placements, rect)
            assert over == 0
            assert colour_shift == (2 if sparse else 7) and (sparse or listed > 0)
            assert got == want, f"{name}: the sub-world blob of {rect} differs from the model's ({len(got)} vs {len(want)} bytes)"
            checked += 1
    finally:
        ws.close()
    assert checked == len(world_cases(dims)) - 1


# ---- layouts and entry points ------------------------------------------------------------------------------------------------------------------

def test_copy_fails_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    p = gpu.copy_placements_array([_placement((0, 0, 0), (1, 1, 1), (2, 0, 0))])
    ms = C.c_float()
    assert L.cvx_world_copy(None, p.ctypes.data, 1, 0, C.byref(ms)) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    # a context without a device or world (tests/copy_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 12 + [-3], codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_copy(h, p.ctypes.data, 1, 0, C.byref(ms)) == -3
        finally:
            L.cvx_destroy(h)


def test_copy_placements_array_accepts_dicts_and_structured_arrays():
    a = gpu.copy_placements_array([{"srcMin": (1, 2, 3), "srcMax": (4, 5, 6), "dst": (-7, 8, 9)},
                                   {"srcMin": (0, 0, 0), "srcMax": (2, 2, 2), "dst": (1, 1, 1), "transform": 13, "op": gpu.BRUSH_PAINT, "move": True}])
    assert a.dtype == gpu.COPY_PLACEMENT_DTYPE and a.flags.c_contiguous
    assert a["op"].tolist() == [gpu.COPY_REPLACE, gpu.BRUSH_PAINT] and a["transform"].tolist() == [0, 13] and a["move"].tolist() == [0, 1]
    assert (gpu.copy_placements_array(a) == a).all()
    raw = a.tobytes()
    assert struct.unpack_from("<12i", raw, 0) == (1, 2, 3, 4, 5, 6, -7, 8, 9, 0, 3, 0)
    assert struct.unpack_from("<12i", raw, 48) == (0, 0, 0, 2, 2, 2, 1, 1, 1, 13, 2, 1)
