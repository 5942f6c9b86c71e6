"""CPU (no GPU needed): the rules behind cvx_world_settle (cpuvox_amd/csrc/cvx_settle.h), compiled for the host through tests/settle_rules.cpp
(which drives them with a sequential union-find and a Bellman-Ford over the node constraints), against the independent dense model of
tests/settlemodel.py, which knows only the contract's step rule.

- World mode: the worlds of the pieces test (records with 1 .. 3 runs, run-list columns, foreign columns with split runs, both colour layouts)
  uploaded into a host-only context; the named boxes plus 40 random boxes and anchor masks each with maxDrop from {0, 1, 3}: the summary, the list,
  the drops and the decoded sub-world blob of the settle's rectangle equal the model's exactly, and the model changes nothing outside it.
- Constructed shapes: a stack of twelve slabs, two interlocked pieces, a table stopped by a pole under one column.
- Every INVALID_ARGUMENT case without a world (the header's mirrors: tests/test_abi_mirrors.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import piecesmodel
import ruleslib
import settlemodel
from cpuvox_amd import gpu, host
from test_world_brush_cpu import _pick_world
from test_world_pieces_cpu import GROUND, pieces_rows, world_boxes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY_NAMES = ("floatingPieces", "floatingVoxels", "fallenPieces", "fallenVoxels", "largestDrop")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("settle_rules", tmp_path_factory.mktemp("settle"))


def settle_rectangle(pieces, drops, dims, level_count):
    """cvx_world_settle's rectangle (x0, z0, sizeX, sizeZ): that of the pieces with drop > 0, or None when nothing falls."""
    return piecesmodel.rectangle(pieces[drops > 0], dims, level_count)


def run_world(rules, tmp_path, ws, box_min, box_max, anchors, max_drop, level_count):
    """tests/settle_rules.cpp `world` on LOD 0 of ws -> (summary dict, pieces, drops, rectangle, blob bytes, over, nodes, sweeps, ms)."""
    info = ws.info(0)
    blob, lst, out = tmp_path / "world.bin", tmp_path / "list.bin", tmp_path / "sub.bin"
    if not blob.exists():
        blob.write_bytes(ws.storage(0).tobytes())
    text = subprocess.check_output([rules, "world", str(blob), str(info.dimX), str(info.dimY), str(info.dimZ), str(info.columnCount),
                                    *[str(int(v)) for v in box_min], *[str(int(v)) for v in box_max], str(anchors), str(max_drop), str(level_count), str(lst), str(out)],
                                   text=True)
    m = re.match(r"colorShift (\d+) listed (\d+) over (\d+) rect (\d+) (\d+) (\d+) (\d+) nodes (\d+) sweeps (\d+) ms ([0-9.]+)", text)
    assert m, text
    raw = lst.read_bytes()
    summary = np.frombuffer(raw[:40], dtype=gpu.SETTLE_SUMMARY_DTYPE)[0]
    count = (len(raw) - 40) // 52
    pieces = np.frombuffer(raw[40:40 + 48 * count], dtype=gpu.PIECE_DTYPE)
    drops = np.frombuffer(raw[40 + 48 * count:], dtype=np.int32)
    return ({n: int(summary[n]) for n in SUMMARY_NAMES}, pieces, drops, tuple(int(m.group(k)) for k in range(4, 8)), out.read_bytes(), int(m.group(3)),
            int(m.group(8)), int(m.group(9)), float(m.group(10)))


@pytest.mark.parametrize("dims,sparse,level_count,seed", [((32, 32, 32), False, 3, 1), ((16, 64, 32), False, 0, 2), ((32, 128, 32), True, 5, 3)])
def test_settled_rectangle_equals_the_step_model(rules, tmp_path, dims, sparse, level_count, seed):
    rng = np.random.default_rng(seed)
    solid, colour, ws = _pick_world(rng, dims, sparse)
    colour = np.where(solid, colour, 0).astype(colour.dtype)
    cases = [(name, box_min, box_max, anchors) for name, (box_min, box_max, anchors) in world_boxes(dims).items()]
    rng = np.random.default_rng(seed + 100)
    for k in range(40):
        while True:
            box_min = [int(rng.integers(-2, dims[a])) for a in range(3)]
            box_max = [int(rng.integers(box_min[a] + 1, dims[a] + 3)) for a in range(3)]
            if piecesmodel.clip_box(dims, box_min, box_max) is not None:
                break
        cases.append((f"random box {k}", box_min, box_max, int(rng.integers(0, 8))))
    fell = capped = 0
    try:
        for k, (name, box_min, box_max, anchors) in enumerate(cases):
            max_drop = (0, 1, 3)[k % 3] if k < 8 else int(rng.choice([0, 1, 3]))
            label = f"{name} {box_min} {box_max} anchors {anchors} maxDrop {max_drop}"
            want_pieces, want_drops, want_summary, (s, c) = settlemodel.settle(solid, colour, box_min, box_max, anchors, max_drop)
            summary, pieces, drops, rect, got, over, _, _, _ = run_world(rules, tmp_path, ws, box_min, box_max, anchors, max_drop, level_count)
            assert over == 0, label
            assert summary == want_summary, label
            assert pieces_rows(pieces) == pieces_rows(want_pieces), label
            assert drops.tolist() == want_drops.tolist(), label
            want_rect = settle_rectangle(want_pieces, want_drops, dims, level_count)
            if want_rect is None:
                assert got == b"" and (s == solid).all() and (c == colour).all(), label
                continue
            assert rect == want_rect, label
            x0, z0, sx, sz = rect
            got_solid, got_colour = piecesmodel.decode_blob(got, (sx, dims[1], sz))
            assert (got_solid == s[x0:x0 + sx, :, z0:z0 + sz]).all(), f"{label}: occupancy differs"
            assert (got_colour == c[x0:x0 + sx, :, z0:z0 + sz]).all(), f"{label}: colours differ"
            outside = np.ones(dims, dtype=bool)
            outside[x0:x0 + sx, :, z0:z0 + sz] = False
            assert (s[outside] == solid[outside]).all() and (c[outside] == colour[outside]).all(), f"{label}: the model moved something outside the rectangle"
            fell += 1
            capped += max_drop > 0 and want_summary["largestDrop"] == max_drop
    finally:
        ws.close()
    assert fell >= 8 and capped >= 3, (fell, capped)  # (of 48 cases: the worlds do exercise the fall and the cap)


def test_stacks_cycles_and_ledges(rules, tmp_path):
    """Constructed shapes in one world: twelve slabs with 1 .. 12 voxels of air under them (drop_k = the prefix sum: a sweep per slab), two
    interlocked pieces that hold each other (a cycle in the piece graph), a table stopped by a pole under one column that is not its lowest one."""
    dims = (64, 128, 64)
    solid = np.zeros(dims, dtype=bool)
    solid[:, 0, :] = True
    y = 0
    for k in range(1, 13):
        y += k + 1
        solid[4:8, y, 4:8] = True
    solid[20:25, 20, 20] = solid[20, 10:21, 21] = solid[20:25, 10, 22] = True       # p
    solid[22:27, 18, 20] = solid[26, 12:19, 21] = solid[22:27, 12, 22] = True       # q: under p's upper bar, over p's lower bar
    solid[40:48, 20:22, 40:48] = solid[40, 10:20, 40] = solid[47, 1:16, 47] = True  # the table, its long leg, the pole
    x, yy, z = np.nonzero(solid)
    colour = np.zeros(dims, dtype=np.uint32)
    colour[x, yy, z] = (0xFF000000 | ((x * 2654435761 + yy * 40503 + z * 2246822519) & 0xFFFFFF)).astype(np.uint32)
    ws = host.WorldSet.from_voxels(dims, x.astype(np.int32), yy.astype(np.int32), z.astype(np.int32), colour[x, yy, z], threads=2)
    try:
        for max_drop, want in ((0, [78, 66, 55, 45, 36, 28, 21, 15, 10, 6, 3, 1, 9, 10, 4]), (5, [5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 3, 1, 5, 5, 4])):
            want_pieces, want_drops, want_summary, (s, c) = settlemodel.settle(solid, colour, (0, 0, 0), dims, GROUND, max_drop)
            assert want_drops.tolist() == want, max_drop
            summary, pieces, drops, rect, got, over, _, sweeps, _ = run_world(rules, tmp_path, ws, (0, 0, 0), dims, GROUND, max_drop, 5)
            assert over == 0 and summary == want_summary and pieces_rows(pieces) == pieces_rows(want_pieces) and drops.tolist() == want
            assert sweeps >= 2
            x0, z0, sx, sz = rect
            assert rect == settle_rectangle(want_pieces, want_drops, dims, 5) == (0, 0, 64, 64)
            got_solid, got_colour = piecesmodel.decode_blob(got, (sx, dims[1], sz))
            assert (got_solid == s).all() and (got_colour == c).all(), max_drop
    finally:
        ws.close()


def test_settle_fails_cleanly_without_a_context_or_world(rules):
    L = gpu.lib()
    lo, hi = np.zeros(3, dtype=np.int32), np.full(3, 8, dtype=np.int32)
    ms = C.c_float()
    assert L.cvx_world_settle(None, lo.ctypes.data, hi.ctypes.data, 0, 0, 0, None, None, 0, None, C.byref(ms)) == -1  # CVX_ERR_INVALID_ARGUMENT: no context
    # a context without a device or world (tests/settle_rules.cpp): bad arguments first, then CVX_ERR_NOT_READY
    codes = [int(v) for v in subprocess.check_output([rules, "args"], text=True).split()]
    assert codes == [-1] * 12 + [-3, -3], codes
    h = C.c_void_p()
    if L.cvx_create(0, C.byref(h)) == 0:  # (a machine with a device: the world is missing)
        try:
            assert L.cvx_world_settle(h, lo.ctypes.data, hi.ctypes.data, 0, 0, 0, None, None, 0, None, C.byref(ms)) == -3
        finally:
            L.cvx_destroy(h)
