"""CPU (no GPU needed): the rule behind cvx_world_snapshot_diff (cpuvox_amd/csrc/cvx_snapshot.h), compiled for the host through
tests/snapshot_rules.cpp, against the dense model of tests/snapshotmodel.py.  Everything is integers and bytes: no comparison has a tolerance.

- The column rule on hand-made pairs and on random ones, with and without IGNORE_COLOUR; the arena's side in every encoding a record can have
  (1, 2 and 3 runs in the record, run-list blocks, split solid runs, split air runs, shared colours, air runs alone), column after column and in
  colour blocks, among them the foreign groups of tests/test_world_sequences_later_cpu.py.
- Whole worlds uploaded into a host-only context and compared with an edited world's blob: the list, its order and the summary.
- The same program under the address and undefined-behaviour sanitizers.
- The argument checks that need no device.
- The Python wrappers and the documents (the header's mirrors: tests/test_abi_mirrors.py)."""
import os
import subprocess

import numpy as np
import pytest

import piecesmodel
import ruleslib
import snapshotmodel
from cpuvox_amd import gpu
from test_gpu_world_brush import _box, _brushed, _sphere
from test_gpu_world_sequences import AIR, DIMS
from test_world_brush_cpu import _pick_world
from test_world_light_cpu import model_world
from test_world_sequences_later_cpu import KINDS, foreign_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGNORE = gpu.SNAPSHOT_IGNORE_COLOUR
FILL, CARVE, PAINT = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT
ENCODINGS = ("builder", "split solid run", "split air run", "shared colours")


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    return ruleslib.build("snapshot_rules", tmp_path_factory.mktemp("snapshot"))


# ---- columns: dense (solid[Y], colour[Y], y upward) <-> runs from the top ------------------------------------------------------------------------

def spans_of(solid):
    """Maximal (is_solid, top, bottom) spans from the top, [bottom, top)."""
    out, top = [], len(solid)
    while top > 0:
        bottom = top - 1
        while bottom > 0 and solid[bottom - 1] == solid[top - 1]:
            bottom -= 1
        out.append((bool(solid[top - 1]), top, bottom))
        top = bottom
    return out


def encode(solid, colour, encoding="builder", rng=None):
    """A dense column as (runs [(colorsIndex or AIR, length)] from the top, the colour array, worldMin, worldMax); nothing for the empty column
    in the builder's encoding.  The other encodings hold the same voxels: solid or air runs cut in two, or a run that takes its colours from the
    place of the top run where they are the same words."""
    if not solid.any():
        return [], [], 0, 0
    runs, palette = [], []
    first = None
    for is_solid, top, bottom in spans_of(solid):
        n = top - bottom
        cut = int(rng.integers(1, n)) if rng is not None and n >= 2 else 0
        if not is_solid:
            runs += [(AIR, cut), (AIR, n - cut)] if encoding == "split air run" and cut else [(AIR, n)]
            continue
        words = [int(c) for c in colour[bottom:top][::-1]]  # from the top
        if encoding == "shared colours" and first is not None and words == first[:n]:
            runs.append((0, n))
            continue
        at = len(palette)
        palette += words
        if first is None:
            first = words
        runs += [(at, cut), (at + cut, n - cut)] if encoding == "split solid run" and cut else [(at, n)]
    ys = np.flatnonzero(solid)
    return runs, palette, int(ys[0]), int(ys[-1]) + 1


def case_words(dim_y, stride, colors_base, flags, arena, snapshot):
    """One case of `snapshot_rules column`: the arena's column as encode() gives it, the snapshot's in the builder's encoding."""
    runs, palette, world_min, world_max = arena
    words = [dim_y, stride, colors_base, flags, world_min, world_max, len(runs)]
    for ci, n in runs:
        words += [ci, n]
    words += [len(palette), *palette]
    runs, palette, _, _ = snapshot
    words.append(len(runs))
    for ci, n in runs:
        words += [ci, n]
    return words + [len(palette), *palette]


def run_columns(rules, tmp_path, cases, env=None):
    src, dst = tmp_path / "columns.bin", tmp_path / "columns.out"
    src.write_bytes(np.array([w for case in cases for w in case], dtype=np.uint64).astype(np.uint32).tobytes())
    subprocess.check_call([rules, "column", str(src), str(dst)], env=env)
    out = np.frombuffer(dst.read_bytes(), dtype=np.uint32).reshape(-1, 3)
    assert len(out) == len(cases)
    return [tuple(int(v) for v in row) for row in out]


def model_column(now, then, flags):
    """(voxels, yMin, yMax) of one column pair through the dense model."""
    as_volume = lambda c: (c[0][None, None, :], c[1][None, None, :])
    changes, summary = snapshotmodel.diff(as_volume(then), as_volume(now), flags=flags)
    if not len(changes):
        return (0, 0, 0)
    return summary["changedVoxels"], int(changes[0]["yMin"]), int(changes[0]["yMax"])


def column_of(dim_y, spans, salt=0):
    """A dense column with the [bottom, top) spans solid, every voxel a colour of its own."""
    solid = np.zeros(dim_y, dtype=bool)
    for bottom, top in spans:
        solid[bottom:top] = True
    colour = np.where(solid, 0xFF000000 | ((np.arange(dim_y) * 0x010305 + salt * 0x0B0D11) & 0xFFFFFF), 0).astype(np.uint32)
    return solid, colour


def random_column(rng, dim_y):
    """1 .. 7 solid runs (3 and fewer fit the record, more go to a run-list block); a few colours, so that equal words meet."""
    solid = np.zeros(dim_y, dtype=bool)
    for _ in range(int(rng.integers(0, 8))):
        lo = int(rng.integers(0, dim_y))
        solid[lo:lo + int(rng.integers(1, dim_y // 3))] = True
    colour = np.where(solid, 0xFF000000 | rng.integers(0, 4, dim_y), 0).astype(np.uint32)
    if rng.random() < 0.3 and solid.any():  # the runs below the first repeat its colours: the shared encoding has something to share
        spans = [s for s in spans_of(solid) if s[0]]
        first = colour[spans[0][2]:spans[0][1]][::-1]
        for _, top, bottom in spans[1:]:
            n = min(top - bottom, len(first))
            colour[top - n:top] = first[:n][::-1]
    return solid, colour


def mutated(rng, column):
    solid, colour = column[0].copy(), column[1].copy()
    dim_y = len(solid)
    for _ in range(int(rng.integers(0, 4))):
        lo = int(rng.integers(0, dim_y))
        hi = min(dim_y, lo + int(rng.integers(1, 12)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            solid[lo:hi], colour[lo:hi] = False, 0
        elif kind == 1:
            colour[lo:hi] = np.where(solid[lo:hi], colour[lo:hi], 0xFF00FF00)
            solid[lo:hi] = True
        else:
            colour[lo:hi] = np.where(solid[lo:hi], 0xFF0000FF, 0)
    return solid, colour


def hand_made(dim_y):
    """(name, the world now, the snapshot, changed under flags 0, changed under IGNORE_COLOUR) -- (voxels, yMin, yMax) each."""
    full, empty = column_of(dim_y, [(0, dim_y)]), column_of(dim_y, [])
    two = column_of(dim_y, [(0, 20), (36, 46)])
    top_off = column_of(dim_y, [(0, dim_y - 1)])
    bottom_off = column_of(dim_y, [(1, dim_y)])
    painted = (full[0], full[1].copy())
    painted[1][dim_y // 2] ^= 0x00010000
    carved = column_of(dim_y, [(0, 20), (36, 40), (42, 46)])  # voxels 40, 41 out of the upper run: every colour index below them shifts
    hole = column_of(dim_y, [(0, 30), (31, dim_y)])
    return [
        ("identical", two, two, (0, 0, 0), (0, 0, 0)),
        ("empty vs empty", empty, empty, (0, 0, 0), (0, 0, 0)),
        ("empty vs solid", empty, two, (30, 0, 46), (30, 0, 46)),
        ("solid vs empty", two, empty, (30, 0, 46), (30, 0, 46)),
        ("a difference at y = 0 alone", bottom_off, full, (1, 0, 1), (1, 0, 1)),
        ("a difference at y = dimY - 1 alone", top_off, full, (1, dim_y - 1, dim_y), (1, dim_y - 1, dim_y)),
        ("a colour in the middle of a long run", painted, full, (1, dim_y // 2, dim_y // 2 + 1), (0, 0, 0)),
        ("a carve that shifts the colour indices below it", carved, two, (2, 40, 42), (2, 40, 42)),
        ("a full column with one voxel out", hole, full, (1, 30, 31), (1, 30, 31)),
        ("a full column against the one with a voxel out", full, hole, (1, 30, 31), (1, 30, 31)),
    ]


def check_hand_made_pairs(rules, tmp_path, env=None):
    cases, want, names = [], [], []
    for dim_y in (64, 256):
        for name, now, then, plain, ignoring in hand_made(dim_y):
            assert model_column(now, then, 0) == plain and model_column(now, then, IGNORE) == ignoring, f"{name}: the model"
            for encoding in ENCODINGS:
                for stride, base in ((1, 32), (32, 96)):
                    for flags, expected in ((0, plain), (IGNORE, ignoring)):
                        arena = encode(*now, encoding, np.random.default_rng(len(cases)))
                        cases.append(case_words(dim_y, stride, base, flags, arena, encode(*then)))
                        want.append(expected)
                        names.append((dim_y, name, encoding, stride, flags))
    got = run_columns(rules, tmp_path, cases, env)
    bad = [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    assert not bad, bad[:5]
    assert len(cases) == 2 * 10 * 4 * 2 * 2


def test_the_column_rule_on_the_hand_made_pairs(rules, tmp_path):
    check_hand_made_pairs(rules, tmp_path)


def test_the_column_rule_on_random_pairs_in_every_encoding(rules, tmp_path):
    rng = np.random.default_rng(17)
    cases, want, seen = [], [], {e: 0 for e in ENCODINGS}
    kinds = {"unchanged": 0, "changed": 0, "colour only": 0, "listed": 0, "in the record": 0, "shared": 0}
    for k in range(1500):
        dim_y = (64, 256)[k % 2]
        then = random_column(rng, dim_y)
        now = mutated(rng, then) if k % 5 else then
        encoding = ENCODINGS[k % 4]
        arena = encode(*now, encoding, rng)
        solid_runs = sum(1 for ci, _ in arena[0] if ci != AIR)
        kinds["listed" if solid_runs > 3 else "in the record"] += 1
        kinds["shared"] += encoding == "shared colours" and any(ci == 0 for ci, _ in arena[0][1:] if ci != AIR) and solid_runs > 1
        stride, base = ((1, 40), (32, 128))[(k // 4) % 2]
        plain, ignoring = model_column(now, then, 0), model_column(now, then, IGNORE)
        kinds["unchanged" if plain == (0, 0, 0) else "changed"] += 1
        kinds["colour only"] += plain != (0, 0, 0) and ignoring == (0, 0, 0)
        for flags, expected in ((0, plain), (IGNORE, ignoring)):
            cases.append(case_words(dim_y, stride, base, flags, arena, encode(*then)))
            want.append(expected)
        seen[encoding] += 1
    assert min(kinds.values()) >= 20, kinds
    got = run_columns(rules, tmp_path, cases)
    bad = [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:5])


def test_the_foreign_groups_compare_equal_to_their_own_voxels(rules, tmp_path):
    """The columns the sequence tests upload with cvx_world_set_columns, each against the builder's encoding of the voxels it decodes to (no
    change: the encoding differs and the voxels do not) and against those voxels with one painted and one carved."""
    cases, want = [], []
    for k, kind in enumerate(KINDS):
        blob = foreign_blob(kind, 7 + k)
        words = np.frombuffer(blob, dtype=np.uint32)
        run_count = int(words[1] & 0xFFFF)
        runs = [(int(w & 0xFFFF), int(w >> 16)) for w in words[4:4 + run_count]]
        palette = [int(c) for c in words[5 + run_count:]]
        solid, colour = (a[0, :, 0] for a in piecesmodel.decode_blob(blob, (1, DIMS[1], 1)))
        arena = (runs, palette, int(words[1] >> 16), int(words[2]))
        edited = (solid.copy(), colour.copy())
        if solid.any():
            edited[1][40] ^= 0x00000100
            edited[0][5], edited[1][5] = False, 0
        for then in ((solid, colour), edited):
            for stride, base in ((1, 32), (32, 64)):
                for flags in (0, IGNORE):
                    cases.append(case_words(DIMS[1], stride, base, flags, arena, encode(*then)))
                    want.append(model_column((solid, colour), then, flags))
    got = run_columns(rules, tmp_path, cases)
    assert got == want, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    assert want.count((0, 0, 0)) == 4 * 4 + 4, "the foreign columns equal their voxels; the all-air column has nothing to edit"
    assert (2, 5, 41) in want and (1, 5, 6) in want


# ---- whole worlds ------------------------------------------------------------------------------------------------------------------------------------

def as_xzy(solid, colour):
    return solid.transpose(0, 2, 1), np.where(solid, colour, 0).transpose(0, 2, 1)


def run_world(rules, tmp_path, arena_ws, dims, snapshot_blob, rect, flags, env=None):
    a, b, out = tmp_path / "arena.bin", tmp_path / "snapshot.bin", tmp_path / "diff.out"
    a.write_bytes(arena_ws.storage(0).tobytes())
    b.write_bytes(snapshot_blob)
    subprocess.check_call([rules, "world", str(a), *[str(d) for d in dims], str(arena_ws.info(0).columnCount), str(b), *[str(v) for v in rect], str(flags), str(out)],
                          env=env, stdout=subprocess.DEVNULL)
    raw = np.frombuffer(out.read_bytes(), dtype=np.int32)
    summary = {"changedColumns": int(raw[0]) | int(raw[1]) << 32, "changedVoxels": int(raw[2]) | int(raw[3]) << 32, "min": tuple(raw[4:7].tolist()),
               "max": tuple(raw[7:10].tolist())}
    return raw[10:].view(snapshotmodel.CHANGE_DTYPE), summary


EDITS = [_sphere(CARVE, (60, 14, 66), 9), _box(FILL, (20, 0, 24), (24, 58, 30), 0xFF2040F0), _box(PAINT, (90, 0, 90), (91, 64, 91), 0xFF101010),
         _box(CARVE, (5, 0, 5), (6, 1, 6)), _box(FILL, (7, 63, 9), (8, 64, 10), 0xFF445566)]
RECTS = [(0, 0, DIMS[0], DIMS[2]), (50, 55, 21, 23), (20, 24, 1, 1), (100, 100, 8, 8)]


def check_worlds(rules, tmp_path, sparse, env=None):
    """The arena holds the EDITED world as cvx_world_upload lays it out (records with 1 .. 3 runs, run-list blocks; colour blocks, or column
    after column when sparse), the snapshot is the world before the edits."""
    solid, colour, before = _pick_world(np.random.default_rng(23), DIMS, sparse)
    after_dense = _brushed(solid, colour, EDITS)
    after = model_world(DIMS, *after_dense)
    try:
        changed_somewhere = 0
        for rect in RECTS:
            x0, z0, sx, sz = rect
            cut = lambda v: tuple(a[x0:x0 + sx, z0:z0 + sz] for a in as_xzy(*v))
            for flags in (0, IGNORE):
                want, want_summary = snapshotmodel.diff(cut((solid, colour)), cut(after_dense), (x0, z0), flags)
                got, summary = run_world(rules, tmp_path, after, DIMS, before.extract_region(0, *rect)[0], rect, flags, env)
                assert summary == want_summary, (rect, flags, summary, want_summary)
                assert got.tobytes() == want.tobytes(), (rect, flags)
                changed_somewhere += len(want) > 0
        assert changed_somewhere >= (2 if sparse else 5), "the sparse world has nothing under the sphere"
        whole, summary = snapshotmodel.diff(as_xzy(solid, colour), as_xzy(*after_dense))
        painted = whole[(whole["x"] == 90) & (whole["z"] == 90)]
        assert len(painted) == 1 or sparse, "the painted column"
        assert summary["min"][1] == 0 and summary["max"][1] == DIMS[1], "the one-voxel carve at y = 0 and the fill at y = dimY - 1"
        ignoring = snapshotmodel.diff(as_xzy(solid, colour), as_xzy(*after_dense), flags=IGNORE)[1]["changedVoxels"]
        assert ignoring < summary["changedVoxels"] or (sparse and ignoring == summary["changedVoxels"])
    finally:
        before.close()
        after.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_worlds_against_the_model_list_order_and_summary(rules, tmp_path, sparse):
    check_worlds(rules, tmp_path, sparse)


def test_the_rules_are_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same stand-alone program (its own main; nothing is loaded into Python) built with -fsanitize=address,undefined: the hand-made pairs,
    a world and the argument checks run to the end with the same results."""
    out = ruleslib.build("snapshot_rules", tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # (the HIP runtime the library links keeps its own allocations to the end)
    check_hand_made_pairs(out, tmp_path, env)
    check_worlds(out, tmp_path, False, env)
    assert len(subprocess.check_output([out, "args"], text=True, env=env).splitlines()) == 12


# ---- the argument checks ----------------------------------------------------------------------------------------------------------------------------

def test_the_rejections_that_need_no_device(rules):
    lines = [line.split("|", 1) for line in subprocess.check_output([rules, "args"], text=True).splitlines()]
    got = [(int(code), message) for code, message in lines]
    want = [
        (-1, ""), (-1, "cvx_world_snapshot: out is NULL"), (-1, "levelCount 6 outside 0 .. 5"), (-1, "levelCount -1 outside 0 .. 5"),
        (-3, "world LOD 0 has not been uploaded"),
        (-1, ""), (-1, ""),
        (-1, ""), (-1, "cvx_world_snapshot_restore: snap is NULL"),
        (-1, ""), (-1, "cvx_world_snapshot_diff: snap is NULL"), (-1, "cvx_world_snapshot_diff_device: snap is NULL"),
    ]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w] or (len(got), len(want))


def test_python_wrappers():
    assert hasattr(gpu.Context, "world_snapshot") and all(hasattr(gpu.Snapshot, n) for n in ("restore", "diff", "diff_device", "close", "__enter__", "__exit__"))
    assert "destroyed before" in gpu.Snapshot.__doc__


# ---- wrappers and documents -------------------------------------------------------------------------------------------------------------------------------------------

def test_the_documents_name_the_calls():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert f"all {len(gpu.EXPORTS)} exports" in readme
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("tools", "README.md"), os.path.join("profiles", "snapshot.md")):
        assert "cvx_world_snapshot" in open(os.path.join(ROOT, name)).read(), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "cvx_world_snapshot_restore" in integration and "undo" in integration
