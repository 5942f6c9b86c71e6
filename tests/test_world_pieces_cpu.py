"""CPU (no GPU needed): the rules behind cvx_world_pieces (cpuvox_amd/csrc/cvx_pieces.h), compiled for the host through tests/pieces_rules.cpp
(which drives them with a sequential union-find), against the independent dense model of tests/piecesmodel.py (scipy.ndimage.label).

- Column mode: 2000 random small worlds (seed 2031) of up to 4 x 4 random columns (records with 1..3 runs and listed columns, both colour
  layouts, foreign encodings with split runs and shared colours) with random boxes (partly outside the world) and anchor masks: the summary,
  the ordered floating list and every column of the world without the floating pieces (runs, colours, worldMin / worldMax in the builder's
  encoding) must equal the model's exactly.
- World mode: small worlds uploaded into a host-only context; list and summary equal the model's and the sub-world blob of the REMOVE rectangle
  equals, byte for byte, the same rectangle of the model's world built on the host.
- The call without a context / world and every INVALID_ARGUMENT case (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import piecesmodel
import pyworld
import ruleslib
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world, _random_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUND, OUTSIDE, LARGEST = gpu.ANCHOR_GROUND, gpu.ANCHOR_OUTSIDE, gpu.ANCHOR_LARGEST


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("pieces_rules", tmp_path_factory.mktemp("pieces"))


def pieces_rows(pieces):
    """A PIECE_DTYPE array as plain rows (min, max, seed, voxels) for comparisons and messages."""
    return [(p["min"].tolist(), p["max"].tolist(), p["seed"].tolist(), int(p["voxels"])) for p in pieces]


# ---- column mode -------------------------------------------------------------------------------------------------------------------------------

def _model_case(solid, colour, box_min, box_max, anchors):
    pieces, summary, mask = piecesmodel.analyse(solid, box_min, box_max, anchors)
    s = solid & ~mask
    gx, dim_y, gz = solid.shape
    columns = []
    for x in range(gx):
        for z in range(gz):
            ys = np.nonzero(s[x, :, z])[0][::-1]
            col = pyworld.final_column([(int(y), int(colour[x, y, z])) for y in ys], dim_y - 1, 1)
            if col is None:
                columns.append((False, [], [], 0, 0))
                continue
            runs, colours, wmin, wmax = col
            columns.append((False, [((ci & 0xFFFF) | (n << 16)) for ci, n in runs], list(colours), wmin, wmax))
    return summary, pieces_rows(pieces), columns


def _run_columns(rules, tmp_path, cases):
    words = []
    for dim_y, gx, gz, stride, columns, box_min, box_max, anchors in cases:
        words += ruleslib.world_words(dim_y, gx, gz, stride, columns) + list(box_min) + list(box_max) + [anchors]
    out = ruleslib.run_cases(rules, "columns", tmp_path, words)
    results, at = [], 0
    for dim_y, gx, gz, *_ in cases:
        fp, fv, ap, av = [int(v) for v in out[at:at + 4]]
        at += 4
        rows = []
        for _ in range(fp):
            w = out[at:at + 10].astype(np.int32).tolist()
            at += 10
            rows.append((w[0:3], w[3:6], w[6:9], w[9]))
        columns, at = ruleslib.edited_columns(out, at, gx * gz)
        results.append(({"floatingPieces": fp, "floatingVoxels": fv, "anchoredPieces": ap, "anchoredVoxels": av}, rows, columns))
    assert at == len(out)
    return results


def test_rules_match_the_dense_model_on_random_small_worlds(rules, tmp_path):
    rng = np.random.default_rng(2031)
    cases, models = [], []
    split = listed_like = floating = anchored = multi = 0
    for _ in range(2000):
        dim_y = int(rng.choice([8, 16, 64, 256]))
        gx, gz = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        stride = int(rng.choice([1, 32]))
        solid = np.zeros((gx, dim_y, gz), dtype=bool)
        colour = np.zeros((gx, dim_y, gz), dtype=np.uint32)
        columns = []
        for k in range(gx * gz):
            runs, colours, _, dense = _random_column(rng, dim_y)
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
        colour[~solid] = 0
        dims = (gx, dim_y, gz)
        while True:
            box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
            box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
            if piecesmodel.clip_box(dims, box_min, box_max) is not None:
                break
        if rng.random() < 0.3:
            box_min, box_max = [0, 0, 0], list(dims)
        anchors = int(rng.integers(0, 8))
        cases.append((dim_y, gx, gz, stride, columns, box_min, box_max, anchors))
        models.append(_model_case(solid, colour, box_min, box_max, anchors))
        floating += models[-1][0]["floatingPieces"]
        anchored += models[-1][0]["anchoredPieces"]
        multi += models[-1][0]["floatingPieces"] + models[-1][0]["anchoredPieces"] > 2
    results = _run_columns(rules, tmp_path, cases)
    bad = [i for i, (got, want) in enumerate(zip(results, models)) if got != want]
    if bad:
        i = bad[0]
        part = next(k for k in range(3) if results[i][k] != models[i][k])
        raise AssertionError(f"{len(bad)} of {len(cases)} cases differ; first: case {i} {cases[i]}\n got {results[i][part]}\nwant {models[i][part]}")
    assert split > 100 and listed_like > 300 and floating > 2000 and anchored > 1000 and multi > 500, (split, listed_like, floating, anchored, multi)


# ---- world mode ---------------------------------------------------------------------------------------------------------------------------------

def run_world(rules, tmp_path, ws, box_min, box_max, anchors, level_count):
    """tests/pieces_rules.cpp `world` on LOD 0 of ws -> (summary dict, pieces array, rectangle, blob bytes, colorShift, listed, over, nodes, ms)."""
    info = ws.info(0)
    blob, lst, out = tmp_path / "world.bin", tmp_path / "list.bin", tmp_path / "sub.bin"
    blob.write_bytes(ws.storage(0).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                    *[str(int(v)) for v in box_min], *[str(int(v)) for v in box_max], str(anchors), str(level_count), str(lst), str(out)], text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) over (\d+) rect (\d+) (\d+) (\d+) (\d+) nodes (\d+) ms ([0-9.]+)", text)
    assert m, text
    raw = lst.read_bytes()
    summary = np.frombuffer(raw[:32], dtype=gpu.PIECES_SUMMARY_DTYPE)[0]
    pieces = np.frombuffer(raw[32:], dtype=gpu.PIECE_DTYPE)
    return ({n: int(summary[n]) for n in gpu.PIECES_SUMMARY_DTYPE.names}, pieces, tuple(int(m.group(k)) for k in range(4, 8)), out.read_bytes(),
            int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(8)), float(m.group(9)))


def world_boxes(dims):
    """Named (box_min, box_max, anchors) over a world of `dims` (the GPU test uses them too)."""
    dx, dy, dz = dims
    return {
        "whole world, ground": ((0, 0, 0), dims, GROUND),
        "whole world, largest": ((0, 0, 0), dims, LARGEST),
        "whole world, nothing anchored": ((0, 0, 0), dims, 0),
        "inner box, outside": ((3, 2, 5), (dx - 4, dy - 3, dz - 2), OUTSIDE),
        "inner box, nothing anchored": ((3, 2, 5), (dx - 4, dy - 3, dz - 2), 0),
        "upper half, outside and largest": ((0, dy // 4, 0), (dx, dy, dz), OUTSIDE | LARGEST),
        "partly outside the world": ((-5, -3, dz // 2), (dx // 2, dy + 9, dz + 4), GROUND | OUTSIDE),
        "one column": ((3, 0, 1), (4, dy, 2), GROUND),
    }


@pytest.mark.parametrize("dims,sparse,level_count,seed", [((32, 32, 32), False, 3, 1), ((16, 64, 32), False, 0, 2), ((32, 128, 32), True, 5, 3)])
def test_removed_rectangle_equals_the_model_world(rules, tmp_path, dims, sparse, level_count, seed):
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    removed = 0
    try:
        for name, (box_min, box_max, anchors) in world_boxes(dims).items():
            want_pieces, want_summary, mask = piecesmodel.analyse(solid, box_min, box_max, anchors)
            summary, pieces, rect, got, colour_shift, listed, over, _, _ = run_world(rules, tmp_path, ws, box_min, box_max, anchors, level_count)
            assert colour_shift == (2 if sparse else 7) and (sparse or listed > 0) and over == 0
            assert summary == want_summary, name
            assert pieces_rows(pieces) == pieces_rows(want_pieces), name
            want_rect = piecesmodel.rectangle(want_pieces, dims, level_count)
            if want_rect is None:
                assert got == b"", name
                continue
            assert rect == want_rect, name
            s, c = piecesmodel.remove(solid, colour, box_min, box_max, anchors)
            x, y, z = np.nonzero(s)
            want_ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), c[x, y, z], threads=2)
            try:
                want, _ = want_ws.extract_region(0, *rect)
            finally:
                want_ws.close()
            assert got == want, f"{name}: the sub-world blob of {rect} differs from the model's ({len(got)} vs {len(want)} bytes)"
            removed += 1
    finally:
        ws.close()
    assert removed >= 4


# ---- layouts and entry points ------------------------------------------------------------------------------------------------------------------

def test_pieces_fails_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    lo, hi = np.zeros(3, dtype=np.int32), np.full(3, 8, dtype=np.int32)
    ms = C.c_float()
    assert L.cvx_world_pieces(None, lo.ctypes.data, hi.ctypes.data, 0, 0, 0, None, 0, None, C.byref(ms)) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    # a context without a device or world (tests/pieces_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 13 + [-3], codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_pieces(h, lo.ctypes.data, hi.ctypes.data, 0, 0, 0, None, 0, None, C.byref(ms)) == -3
        finally:
            L.cvx_destroy(h)
