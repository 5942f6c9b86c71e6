"""CPU: the call lists of tests/test_gpu_world_sequences_later.py, run on the calls' dense models alone.

The GPU file runs the newer world calls -- stamp, copy, cvx_world_write_heights, cvx_world_place_models, cvx_world_write_voxels, cavities FILL,
cvx_world_light_lamps, the brush's capsules and ellipsoids, and the readers surface, distance, spread, nav, cavities REPORT, read_voxels,
read_heights, read_model -- one after another on one arena.  Its call lists are DATA, written here: a plan is a list of (call, arguments), and
`Models` holds, per call, the model the call's own test uses, on ONE (solid, colour) volume.  A plan runs on the models alone (ModelRun, here) or
on a context beside them (the GPU file's subclass of _Sequence, which takes these methods and the same lists).

What a case is named for is asserted from the models, so a plan is known to be valid where there is no device: every writer changes the volume;
in the editor's loop every writer changes a column the writer before it changed; a spread reaches voxels the step before it carved; the model
place has an instance list longer than a wave whose instances over one column are every other one, FILL and CARVE, and their order matters; the
foreign columns' runs touch, their colours are shared, the readers' boxes sit where the encoding matters; the terrain that must not fit the
tails needs more colours than the headroom rule leaves (relayout_need).  Seeds, boxes and lists are constants."""
import numpy as np
import pytest
from scipy import ndimage

import cavitymodel
import copymodel
import densemodel
import distancemodel
import heightsmodel
import lampmodel
import liftmodel
import lightmodel
import modelsmodel
import navmodel
import piecesmodel
import shapemodel
import snapshotmodel
import spreadmodel
import stampmodel
import surfacemodel
from cpuvox_amd import gpu, host
from test_gpu_world_brush import _box, _brushed, _dense
from test_gpu_world_dense import TALL, _boundaries, _tall_solid
from test_gpu_world_sequences import AIR, DIMS, FOREIGN, SETUP, STROKES, _foreign_blob
from test_world_brush_cpu import _pick_world
from test_world_heights_cpu import WALLED, write_box
from test_world_light_cpu import ALPHA, RGB
from test_world_models_cpu import as_dicts, identity_at, quarter_forward

FILL, CARVE, PAINT, REPLACE = gpu.BRUSH_FILL, gpu.BRUSH_CARVE, gpu.BRUSH_PAINT, gpu.COPY_REPLACE
CAPSULE, ELLIPSOID = gpu.SHAPE_CAPSULE, gpu.SHAPE_ELLIPSOID
IGNORE = gpu.SURFACE_IGNORE_COLOUR
TO_SOLID, TO_AIR, SIGNED = gpu.DISTANCE_TO_SOLID, gpu.DISTANCE_TO_AIR, gpu.DISTANCE_SIGNED
SPREAD_AIR, SPREAD_SOLID = gpu.SPREAD_AIR, gpu.SPREAD_SOLID
UP_AND_DOWN = 0x0C  # spread's stepFaces: -Y and +Y alone
WRITERS = ("brush", "shapes", "stamp", "copy", "write_heights", "place_models", "write_voxels", "fill_cavities", "lamps", "set_column",
           "lift_remove", "place_lifted", "snapshot_restore", "light")
# (shapes: the brush with capsules and ellipsoids, through tests/shapemodel.py as tests/test_gpu_world_shapes.py does -- pickmodel.apply_strokes, the
# model of `brush`, knows boxes and spheres alone)


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """(a directory, the stamp's triangle rule compiled for the host): what stampmodel.voxelise takes."""
    d = tmp_path_factory.mktemp("later")
    return d, stampmodel.rules(d)


def _columns(rect, dims):
    """bool[dimX, dimZ] of a rectangle (x0, z0, sizeX, sizeZ)."""
    out = np.zeros((dims[0], dims[2]), dtype=bool)
    out[rect[0]:rect[0] + rect[2], rect[1]:rect[1] + rect[3]] = True
    return out


def read_map(dims, src_min, size, transform):
    """The instance whose toModel maps the voxels of a model of the returned size onto the world box at src_min of `size` turned by
    cvx_world_copy's `transform` (0: as it lies), as tests/test_gpu_world_models.py builds it: (the model's size, the instance)."""
    forward, dst_size = quarter_forward(transform, size, (0, 0, 0))
    matrix = np.concatenate([forward[:, :3], (forward[:, 3] - forward[:, :3] @ np.array(src_min, dtype=np.float64))[:, None]], axis=1)
    return dst_size, gpu.model_instance(matrix, dims)


class Models:
    """The models of the newer calls on one (solid, colour) volume: m_<call>(arguments) asserts what the step is there for and returns the
    model's result -- a writer's is the volume after it, a reader's what the device must return.  Needs self.dims, self.solid, self.colour,
    self.work (the `work` fixture) and self.last = None (the columns the writer before changed)."""

    def changed(self, after, label, overlaps=False):
        """A writer's result must differ from the volume, and with `overlaps` in a column the writer before it changed."""
        cols = ((after[0] != self.solid) | (after[1] != self.colour)).any(axis=1)
        assert cols.any(), f"{label} changes nothing"
        if overlaps:
            assert self.last is not None and (cols & self.last).any(), f"{label} changes no column that the writer before it changed"
        self.before, self.last = (self.solid, self.colour), cols
        return after

    # -- writers --------------------------------------------------------------------------------------------------------------------------------
    def m_brush(self, strokes, label, overlaps=False, **_):
        return self.changed(_brushed(self.solid, self.colour, strokes), label, overlaps)

    def m_shapes(self, strokes, label, overlaps=False, **_):
        s, c = self.solid.copy(), self.colour.copy()
        shapemodel.apply_strokes(s, c, gpu.strokes_array(strokes))
        return self.changed((s, c), label, overlaps)

    def mesh(self, spec):
        return host.Mesh.from_arrays({"position": np.float32(spec["position"]), "rgba": np.uint8(spec["rgba"])}, np.int32(spec["indices"]))

    def m_stamp(self, mesh, op, label, overlaps=False, **_):
        d, rules = self.work
        x, y, z, argb = stampmodel.voxelise(rules, self.mesh(mesh), self.dims, d)
        assert len(x) > 0, label
        return self.changed(stampmodel.apply_stamp(self.solid.copy(), self.colour.copy(), x, y, z, argb, op), label, overlaps)

    def m_copy(self, placements, label, overlaps=False, **_):
        return self.changed(copymodel.apply_copies(self.solid, self.colour, gpu.copy_placements_array(placements)), label, overlaps)

    def m_write_heights(self, write, label, overlaps=False, **_):
        return self.changed(heightsmodel.write(self.solid, self.colour, write_box(write), *write[2:]), label, overlaps)

    def m_place_models(self, models, instances, label, overlaps=False, order_matters=None, **_):
        dicts = as_dicts(instances)
        after = modelsmodel.place(self.solid, self.colour, models, dicts)
        if order_matters is not None:  # a column under FILL and CARVE instances, every other one of a list longer than a wave
            x, z = order_matters
            covering = [k for k, d in enumerate(dicts) if d["box_min"][0] <= x < d["box_max"][0] and d["box_min"][2] <= z < d["box_max"][2]]
            ops = {dicts[k]["op"] for k in covering}
            assert len(dicts) > 64 and max(covering) >= 64 and CARVE in ops and ops & {FILL, REPLACE}, label
            assert any(b - a > 1 for a, b in zip(covering, covering[1:])), f"{label}: the instances over ({x}, {z}) lie apart in the list"
            back = modelsmodel.place(self.solid, self.colour, models, dicts[::-1])
            assert (after[0][x, :, z] != back[0][x, :, z]).any() or (after[1][x, :, z] != back[1][x, :, z]).any(), f"{label}: the order does not matter"
        return self.changed(after, label, overlaps)

    def m_write_voxels(self, write, label, overlaps=False, **_):
        at, argb, mask, op = write
        shape = (argb if argb is not None else mask).shape
        box = (tuple(at), (at[0] + shape[0], at[1] + shape[2], at[2] + shape[1]))
        return self.changed(densemodel.write(self.solid, self.colour, box, argb, mask, op), label, overlaps)

    def m_fill_cavities(self, box, label, open_faces=0x3F, max_voxels=0, argb=0xFF123456, overlaps=False, **_):
        want, summary, _ = cavitymodel.analyse(self.solid, *box, open_faces, max_voxels)
        assert len(want) > 0, f"{label}: the model selects no cavity"
        return self.changed(cavitymodel.fill(self.solid, self.colour, *box, open_faces, max_voxels, argb), label, overlaps)

    def m_lamps(self, p, lamps, label, overlaps=False, **_):
        total, stats = lampmodel.lamp_sum(self.solid, p, lamps)
        assert stats["lit"] > 0, f"{label}: no lamp lights a voxel"
        return self.changed((self.solid, lampmodel.light(self.solid, self.colour, p, lamps, total)), label, overlaps)

    def m_set_column(self, x, z, blob, label, **_):
        solid, colour = self.solid.copy(), self.colour.copy()
        solid[x, :, z], colour[x, :, z] = (a[0, :, 0] for a in piecesmodel.decode_blob(blob, (1, self.dims[1], 1)))
        self.before, self.last = (self.solid, self.colour), _columns((x, z, 1, 1), self.dims)
        return solid, colour

    # -- readers: holds(self, want), where given, asserts what the call is placed for -----------------------------------------------------------
    def m_surface(self, box, label, solid_outside=0x04, flags=0, holds=None):
        want = surfacemodel.surface(self.solid, self.colour, *box, solid_outside, flags)
        assert len(want[0]) > 0, label
        return self.held(want, holds, label)

    def m_distance(self, box, label, R=8, mode=TO_SOLID, solid_outside=0x04, holds=None):
        want = distancemodel.field(self.solid, box, R, mode, solid_outside)
        assert ((want != 0) & (abs(want) != distancemodel.FAR)).any(), f"{label}: no voxel near the surface"
        return self.held(want, holds, label)

    def m_spread(self, box, seeds, medium, label, step_faces=0x3F, max_steps=200, holds=None):
        want = spreadmodel.field(self.solid, *box, seeds, medium, step_faces, max_steps)
        assert want[1]["reached"] > 0, label
        return self.held(want, holds, label)

    def m_nav(self, call, goals, label, holds=None):
        want = navmodel.analyse(self.solid, *call[:6], goals, call[6])
        assert want[1]["reached"] > 0, label
        return self.held(want, holds, label)

    def m_report_cavities(self, box, label, open_faces=0x3F, max_voxels=0, holds=None):
        want, summary, _ = cavitymodel.analyse(self.solid, *box, open_faces, max_voxels)
        return self.held((want, summary), holds, label)

    def m_read_voxels(self, box, label, holds=None):
        want = densemodel.read(self.solid, self.colour, box)
        assert want[1].any() and not want[1].all(), label
        return self.held(want, holds, label)

    def m_read_heights(self, box, label, holds=None):
        return self.held(heightsmodel.read(self.solid, self.colour, box), holds, label)

    def m_read_model(self, src_min, size, transform, label, holds=None):
        dst_size, instance = read_map(self.dims, src_min, size, transform)
        d = modelsmodel.from_struct(instance)
        want = modelsmodel.read(self.solid, self.colour, dst_size, d["m"], d["t"])
        assert want[1].any() and not want[1].all(), label
        if transform == 0:
            dense = densemodel.read(self.solid, self.colour, (src_min, tuple(src_min[i] + size[i] for i in range(3))))
            assert (want[0] == dense[0]).all() and (want[1] == dense[1]).all(), f"{label}: the identity reads the dense box"
        return self.held(want, holds, label)

    # -- the newest calls: cvx_world_lift_pieces and cvx_world_snapshot (tests/test_world_sequences_newest_cpu.py has their plans) ----------------------
    def lifted(self, box, anchors, capacity, voxel_capacity, label):
        """liftmodel's result; voxel_capacity None: exactly what the listed pieces need (the model's result with room for everything is the one
        with exactly that room: the prefix rule stores every listed piece in both).  Something must be stored."""
        want = liftmodel.lift(self.solid, self.colour, *box, anchors, capacity, (1 << 62) if voxel_capacity is None else voxel_capacity)
        if voxel_capacity is None:
            voxel_capacity = want.summary["storedVoxels"]
        assert want.summary["storedPieces"] > 0, f"{label}: no piece is stored"
        return want, voxel_capacity

    def m_lift_copy(self, box, anchors, label, capacity=8192, voxel_capacity=None, holds=None):
        """A reader: -> (liftmodel's Lift, the voxelCapacity of the call)."""
        return self.held(self.lifted(box, anchors, capacity, voxel_capacity, label), holds, label)

    def m_lift_remove(self, box, anchors, label, capacity=8192, voxel_capacity=None, overlaps=False, holds=None, **_):
        """A writer: the world without the stored pieces.  self.lift keeps (the Lift, the voxelCapacity) for the call and for place_lifted."""
        self.lift = self.held(self.lifted(box, anchors, capacity, voxel_capacity, label), holds, label)
        return self.changed(self.lift[0].removed, label, overlaps)

    def largest_lifted(self):
        """The stored piece with the most voxels of the last lift_remove: its index in the list."""
        want = self.lift[0]
        return int(np.argmax(want.pieces["piece"]["voxels"][:want.summary["storedPieces"]]))

    def m_place_lifted(self, offset, label, op=None, overlaps=False, **_):
        """A writer: the largest piece of the last lift_remove placed as it lies, `offset` away from where it was."""
        want, k = self.lift[0], self.largest_lifted()
        piece = want.pieces["piece"][k]
        size = tuple(int(piece["max"][a]) - int(piece["min"][a]) for a in range(3))
        at = tuple(int(piece["min"][a]) + offset[a] for a in range(3))
        argb, mask = want.models[k]
        instance = identity_at(at, size, 0, FILL if op is None else op)
        return self.changed(modelsmodel.place(self.solid, self.colour, [(argb, mask.astype(bool))], as_dicts([instance])), label, overlaps)

    def taken(self):
        """{name: (solid, colour, the held rectangle, levelCount)} of the snapshots of this run."""
        return self.__dict__.setdefault("snapshots", {})

    def m_snapshot(self, name, rect, label, levels=5):
        """Neither reader nor writer: the volume as it is, and the rectangle rounded out to 2^levels and clipped.  (`levels`: the snapshot's
        levelCount, under a name that a run on the models alone does not strip from the arguments.)"""
        k = (1 << levels) - 1
        x0, z0 = max(rect[0], 0) & ~k, max(rect[1], 0) & ~k
        x1, z1 = min((rect[0] + rect[2] + k) & ~k, self.dims[0]), min((rect[1] + rect[3] + k) & ~k, self.dims[2])
        self.taken()[name] = (self.solid, self.colour, (x0, z0, x1 - x0, z1 - z0), levels)

    def m_snapshot_diff(self, name, label, flags=0, holds=None):
        """A reader: snapshotmodel's (changes, summary) of the rectangle now against the snapshot."""
        solid, colour, (x0, z0, sx, sz), _ = self.taken()[name]
        cut = lambda a: a[x0:x0 + sx, :, z0:z0 + sz].transpose(0, 2, 1)  # noqa: E731
        want = snapshotmodel.diff((cut(solid), cut(colour)), (cut(self.solid), cut(self.colour)), (x0, z0), flags)
        return self.held(want, holds, label)

    def m_snapshot_restore(self, name, label, overlaps=False, **_):
        """A writer: the columns of the held rectangle as they were when the snapshot was taken."""
        solid, colour, (x0, z0, sx, sz), _ = self.taken()[name]
        s, c = self.solid.copy(), self.colour.copy()
        s[x0:x0 + sx, :, z0:z0 + sz], c[x0:x0 + sx, :, z0:z0 + sz] = solid[x0:x0 + sx, :, z0:z0 + sz], colour[x0:x0 + sx, :, z0:z0 + sz]
        return self.changed((s, c), label, overlaps)

    def m_light(self, p, label, overlaps=False, **_):
        mask, _ = lightmodel.shades(self.solid, p)
        assert mask.any(), f"{label}: the box holds no voxel"
        return self.changed((self.solid, lightmodel.light(self.solid, self.colour, p)), label, overlaps)

    def m_compact(self, label, **_):
        return None

    def held(self, want, holds, label):
        if holds is not None:
            assert holds(self, want), f"{label}: the model's result lacks what the step is placed for"
        return want


class ModelRun(Models):
    """A plan on the models alone."""

    def __init__(self, dims, solid, colour, work):
        self.dims, self.solid, self.colour, self.work, self.last, self.before, self.steps = dims, solid, colour, work, None, None, 0

    def run(self, plan):
        for call, args in plan:
            args = {k: v for k, v in args.items() if k not in ("level_count", "check")}
            out = getattr(self, "m_" + call)(**args)
            if call in WRITERS:
                self.solid, self.colour = out
            self.steps += 1


def sequence_world(seed, sparse=False):
    """(solid, colour) of _Sequence(seed, sparse)."""
    solid, colour, ws = _pick_world(np.random.default_rng(seed), DIMS, sparse)
    ws.close()
    return solid, colour


def tall_world():
    solid = _tall_solid()
    return solid, _dense(solid)


def strokes_plan(strokes, name="stroke"):
    return [("brush", dict(strokes=[s], label=f"{name} {k}")) for k, s in enumerate(strokes)]


def _argb(shape, salt):
    """Colour words without a zero among them, of `shape`."""
    n = np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape)
    return (0xFF000000 | ((n * 2654435761 + salt * 40503) >> 5) & 0xFFFFFF).astype(np.uint32)


def _capsule(op, a, b, r, argb=0):
    return {"op": op, "shape": CAPSULE, "a": a, "b": b, "radius": r, "argb": argb}


def _ellipsoid(op, c, radii, argb=0):
    return {"op": op, "shape": ELLIPSOID, "a": c, "b": radii, "argb": argb}


def _quad(lo, hi, salt):
    """A slanted quad from (lo.x, lo.y, lo.z) up to (hi.x, hi.y, hi.z), two coloured triangles."""
    position = [[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]]
    rgba = [[(40 + 50 * k + 17 * salt) % 256, (200 - 30 * k) % 256, (90 + 11 * salt * k) % 256, 255] for k in range(4)]
    return dict(position=position, rgba=rgba, indices=[0, 1, 2, 0, 2, 3])


def _hills(at, shape, y0, y1, salt):
    """Heights with slopes and cliffs, a few above and below the window; top and side colours."""
    x, z = np.meshgrid(np.arange(shape[0]) + at[0], np.arange(shape[1]) + at[2], indexing="ij")
    heights = (y0 + (y1 - y0) // 3 + (x * 3 + z * 5 + salt) % 17).astype(np.int32)
    heights[(x + 2 * z) % 11 == 0] = y1 + 4
    heights[(2 * x + z) % 13 == 0] = y0 - 3
    return heights, _argb(shape, salt), _argb(shape, salt + 1)


def _shell(size, salt):
    """(argb, mask) of shape (size, size, size): a closed shell one voxel thick."""
    mask = np.ones((size, size, size), dtype=bool)
    mask[1:-1, 1:-1, 1:-1] = False
    return _argb(mask.shape, salt), mask


def _sun(box, target=RGB, **kw):
    args = dict(sun_dir=(3, 4, 1), sun_level=90, sun_range=64, sky_level=60, sky_range=4, floor_level=10)
    args.update(kw)
    return lightmodel.params(*box, target=target, **args)


def _reaches_what_was_carved(box):
    """holds of a spread through air: it reaches a voxel that was solid before the writer before it."""
    def holds(m, want):
        (x0, y0, z0), (x1, y1, z1) = box
        was = m.before[0][x0:x1, y0:y1, z0:z1].transpose(0, 2, 1)
        return ((want[0] >= 0) & was).any()
    return holds


# ---- A. the editor's loop ---------------------------------------------------------------------------------------------------------------------------

def _chain(at, count, ops):
    """`count` instances, every other one over the columns at `at` -- model 0 (3 x 5 x 3, coloured) with ops[0] and model 1 (2 x 9 x 2, a mask)
    with CARVE in turn, shifted in y -- and the others 40 columns away: the list of a column at `at` is every other instance of a list longer
    than a wave."""
    out = []
    for k in range(count):
        if k % 2:
            out.append(identity_at((at[0] + 40 + k % 5, 6 + (k * 5) % 20, at[2] + 20 + k % 3), (3, 5, 3), 0, FILL))
        elif k % 4 == 0:
            out.append(identity_at((at[0], at[1] + (k * 7) % 30, at[2]), (3, 5, 3), 0, ops[0]))
        else:
            out.append(identity_at((at[0] + 1, at[1] + 2 + (k * 5) % 30, at[2] + 1), (2, 9, 2), 1, CARVE))
    return out


def editor_loop(shift, second):
    """The eight writers of the editor's loop with the readers between them, around (18 .. 64, 20 .. 56) + shift.  second: the loop behind the
    compaction, with other ops."""
    sx, sz = shift
    P = lambda x, y, z: (x + sx, y, z + sz)  # noqa: E731
    tag = "second " if second else ""
    models = [(_argb((3, 3, 5), 3 + second), None), (None, np.ones((2, 2, 9), dtype=bool))]
    heights = _hills(P(40, 6, 34), (14, 13), 6, 44, 5 + second)
    write = (P(40, 6, 34), 44, heights[0], heights[1], heights[2], 3 if second else 2, 0 if second else WALLED, PAINT if second else REPLACE)
    shell = _shell(8, 7 + second)
    dense_at = P(51, 32, 43) if second else P(51, 20, 43)
    cavity_box = (P(48, dense_at[1] - 4, 40), P(64, dense_at[1] + 12, 56))
    lit = (P(50, 0, 42), P(62, 48, 54))
    lamps = [lampmodel.lamp(P(56, dense_at[1] + 11, 48), 8, 255), lampmodel.lamp(P(49, 24, 45), 6, 200)]
    spread_box = (P(38, 0, 32), P(58, 64, 50))
    plan = [
        ("stamp", dict(mesh=_quad(P(18, 30, 22), P(46, 42, 40), second), op=CARVE if second else FILL, label=tag + "stamp", overlaps=second)),
        ("surface", dict(box=(P(16, 0, 20), P(48, 64, 42)), label=tag + "surface behind the stamp")),
        ("copy", dict(placements=[dict(srcMin=list(P(18, 0, 22)), srcMax=list(P(30, 48, 34)), dst=list(P(36, 4, 30)), transform=3 if second else 1,
                                       op=FILL if second else REPLACE, move=second)], label=tag + "copy, a quarter turn", overlaps=True)),
        ("write_heights", dict(write=write, label=tag + "heights write", overlaps=True)),
        ("spread", dict(box=spread_box, seeds=[P(39, 60, 33)], medium=SPREAD_AIR, label=tag + "spread through the air behind the heights write",
                        holds=None if second else _reaches_what_was_carved(spread_box))),
        ("place_models", dict(models=models, instances=_chain(P(50, 10, 42), 70, (REPLACE if second else FILL,)), label=tag + "models place", overlaps=True,
                              order_matters=(P(51, 0, 43)[0], P(51, 0, 43)[2]))),
        ("distance", dict(box=(P(48, 0, 40), P(56, 48, 48)), mode=SIGNED, label=tag + "distance behind the models place")),
        ("write_voxels", dict(write=(dense_at, shell[0], shell[1], FILL if second else REPLACE), label=tag + "dense write with a mask", overlaps=True)),
        ("nav", dict(call=(P(46, 0, 38), P(64, 64, 56), 1, 2, 1, 3, 0), goals=[P(55, 60, 47), P(47, 60, 39)], label=tag + "nav behind the dense write")),
        ("fill_cavities", dict(box=cavity_box, label=tag + "cavities FILL", overlaps=True)),
        ("lamps", dict(p=_sun(lit, ALPHA if second else RGB), lamps=lamps, label=tag + "lamps", overlaps=True)),
        ("read_heights", dict(box=(P(48, 0, 40), P(64, 64, 56)), label=tag + "read_heights behind the lamps")),
        ("read_model", dict(src_min=P(50, 16, 42), size=(10, 16, 12), transform=1, label=tag + "read_model, a quarter turn")),
        ("read_model", dict(src_min=P(50, 16, 42), size=(10, 16, 12), transform=0, label=tag + "read_model, the identity")),
        ("shapes", dict(strokes=[_ellipsoid(FILL, P(55, 30, 48), (9, 4, 6), 0xFF00C0FF)] if second else [_capsule(CARVE, P(46, 30, 40), P(62, 18, 56), 3)],
                        label=tag + ("ellipsoid stroke" if second else "capsule stroke"), overlaps=True)),
    ]
    return plan


LOOP_SETUP = strokes_plan(STROKES[:6])
LOOP_FIRST = editor_loop((0, 0), 0)
LOOP_SECOND = editor_loop((3, 2), 1)


def tall_loop(second):
    """The stepped writers on the 32 x 256 x 32 world -- dense, heights, models and the brush walk a column 64 voxels at a time --, each over
    columns the one before it edited, with runs that end at, start at and cross 64, 128 and 192."""
    spans = [[(10, 64)], [(64, 128)], [(60, 190)], [(0, 64), (65, 128), (129, 192), (193, 256)], [(63, 65), (127, 129), (191, 193)]]
    mask = np.zeros((5, 4, TALL[1]), dtype=bool)
    for k, column in enumerate(spans):
        for lo, hi in column:
            mask[k, :, lo:hi] = True
    assert _boundaries(mask[2, 0]) == {60, 190} and _boundaries(mask[4, 0]) == {63, 65, 127, 129, 191, 193}
    at = (6, 0, 7) if second else (4, 0, 9)
    heights = _hills((2, 30, 5), (12, 11), 30, 200, 9 + second)
    tall_model = (_argb((2, 2, 200), 11 + second), None)
    forward, _ = quarter_forward(1, (2, 200, 2), (at[0] + 1, 20, at[2] + 1))
    tag = "second " if second else ""
    return [
        ("write_voxels", dict(write=(at, _argb(mask.shape, 2 + second), mask, CARVE if second else FILL), label=tag + "dense write across the steps")),
        ("write_heights", dict(write=((2, 30, 5), 200, heights[0], heights[1], heights[2], 5 if second else 0, 0, FILL if second else REPLACE),
                               label=tag + "heights write across the steps", overlaps=True)),
        ("read_heights", dict(box=((0, 0, 0), TALL), label=tag + "read_heights")),
        ("place_models", dict(models=[tall_model, (None, np.ones((1, 1, 130), dtype=bool))],
                              instances=[gpu.model_instance(forward, (2, 200, 2), 0, REPLACE if second else FILL), identity_at((at[0] + 2, 62, at[2] + 2), (1, 130, 1), 1, CARVE)],
                              label=tag + "models place across the steps", overlaps=True)),
        ("read_voxels", dict(box=((0, 0, 0), TALL), label=tag + "read_voxels")),
        ("shapes", dict(strokes=[_capsule(FILL if second else CARVE, (at[0] + 3, 250, at[2] + 2), (at[0] + 1, 5, at[2] + 3), 2, 0xFF8040C0)],
                        label=tag + "capsule across the steps", overlaps=True)),
    ]


# ---- B. each writer behind a compaction -------------------------------------------------------------------------------------------------------------

_B_BOX = ((14, 0, 18), (34, 64, 38))  # around the first tower and the carve that cuts it
_B_HEIGHTS = _hills((16, 4, 20), (15, 14), 4, 50, 21)
_B_SHELL = _shell(8, 23)
BEHIND_A_COMPACTION = {
    "stamp": [("stamp", dict(mesh=_quad((14, 20, 20), (32, 34, 36), 3), op=FILL, label="stamp behind the compaction")),
              ("surface", dict(box=_B_BOX, label="surface over the stamp"))],
    "copy": [("copy", dict(placements=[dict(srcMin=[18, 0, 22], srcMax=[28, 60, 32], dst=[22, 2, 26], transform=2, op=REPLACE, move=1)], label="copy behind the compaction")),
             ("read_voxels", dict(box=_B_BOX, label="read_voxels over the copy"))],
    "dense": [("write_voxels", dict(write=((17, 22, 21), _B_SHELL[0], _B_SHELL[1], REPLACE), label="dense write behind the compaction")),
              ("report_cavities", dict(box=_B_BOX, label="cavities REPORT over the dense write", holds=lambda m, want: 216 in want[0]["voxels"].tolist()))],
    "heights": [("write_heights", dict(write=((16, 4, 20), 50, *_B_HEIGHTS, 2, WALLED, REPLACE), label="heights write behind the compaction")),
                ("read_heights", dict(box=_B_BOX, label="read_heights over the heights write"))],
    "models": [("place_models", dict(models=[(_argb((3, 3, 5), 3), None), (None, np.ones((2, 2, 9), dtype=bool))], instances=_chain((20, 20, 25), 70, (FILL,)),
                                     label="models place behind the compaction", order_matters=(21, 26))),
               ("read_model", dict(src_min=(16, 10, 20), size=(12, 40, 10), transform=3, label="read_model over the models place"))],
    "cavities": [("write_voxels", dict(write=((17, 22, 21), _B_SHELL[0], _B_SHELL[1], REPLACE), label="a shell", level_count=5)),
                 ("compact", dict(label="compaction behind the shell")),
                 ("fill_cavities", dict(box=_B_BOX, label="cavities FILL behind the compaction")),
                 ("distance", dict(box=((16, 20, 20), (26, 32, 30)), mode=TO_AIR, label="distance over the filled shell"))],
    "lamps": [("lamps", dict(p=_sun(((16, 0, 20), (30, 64, 34))), lamps=[lampmodel.lamp((18, 30, 22), 8, 255), lampmodel.lamp((26, 40, 32), 10, 220)],
                             label="lamps behind the compaction")),
              ("spread", dict(box=_B_BOX, seeds=[(22, 2, 27)], medium=SPREAD_SOLID, label="spread through the solid under the lamps"))],
}

# the terrain that does not fit the tails: every column of the world, solid from y = 0 up to 44 .. 56 voxels
_R_HEIGHTS = _hills((0, 0, 0), (DIMS[0], DIMS[2]), 0, 56, 31)
RELAYOUT = [
    ("write_heights", dict(write=((0, 0, 0), 56, np.clip(_R_HEIGHTS[0], 44, 56), _R_HEIGHTS[1], _R_HEIGHTS[2], 0, 0, REPLACE), label="a terrain over the whole footprint")),
    ("place_models", dict(models=[(_argb((3, 3, 5), 3), None), (None, np.ones((2, 2, 9), dtype=bool))], instances=_chain((60, 30, 60), 70, (FILL,)),
                          label="models place behind the relayout", order_matters=(61, 61))),
    ("spread", dict(box=((50, 20, 50), (80, 64, 80)), seeds=[(61, 63, 61)], medium=SPREAD_AIR, label="spread behind the relayout")),
    ("read_heights", dict(box=((40, 0, 40), (90, 64, 90)), label="read_heights behind the relayout")),
]


def relayout_need(old_solid, new_solid, edited):
    """A lower bound, from the volumes alone, of the colour slots a write needs in LOD 0's tail.  Colours lie in blocks of 4 x 8 columns as deep
    as their deepest column; a block that must become deeper moves to the tail whole.  A column 8 or more columns away from every column of
    `edited` (bool[dimX, dimZ]: what earlier edits touched) shares its block with unedited columns alone, so that block is at most `depth` deep,
    the most voxels of an unedited column; where the write leaves such a column more voxels than that, its block moves, and takes the column's
    new colours with it at the least."""
    counts_old, counts_new = old_solid.sum(axis=1), new_solid.sum(axis=1)
    near = np.zeros_like(edited)
    for x, z in np.argwhere(edited):
        near[max(x - 8, 0):x + 9, max(z - 8, 0):z + 9] = True
    depth = int(counts_old[~near].max())
    return int(counts_new[~near & (counts_new > depth)].sum())


def slots_in_use(solid):
    """An upper bound of LOD 0's colour slots behind a compaction: a column's block lies within 7 columns of it and is as deep as its deepest
    column."""
    return int(ndimage.maximum_filter(solid.sum(axis=1), size=15, mode="constant").sum())


def headroom(used_slots):
    """cvx_edit.hip's rule for a tail of colour slots: an eighth of what is in use, 16384 slots at the least."""
    return max(used_slots // 8, 16384)


# ---- C. foreign columns ---------------------------------------------------------------------------------------------------------------------------------

ALL_AIR = ([(AIR, 30), (AIR, 34)], 0)
KINDS = dict(FOREIGN, **{"all air": ALL_AIR})
SPACING = 4  # columns between the foreign columns of a group: room for a tower, a pocket


def foreign_blob(kind, salt):
    runs, colours = KINDS[kind]
    if kind != "all air":
        return _foreign_blob(runs, colours, salt)
    words = [ci | (n << 16) for ci, n in runs]
    return np.array([0, len(runs), 0, 0, *words, 0], dtype=np.uint32).tobytes()  # (worldMin = worldMax = 0: no solid voxel)


def group_columns(at):
    """{kind: (x, z)} of the group at `at`."""
    return {kind: (at[0] + SPACING * k, at[1]) for k, kind in enumerate(KINDS)}


def group_plan(at, salt):
    return [("set_column", dict(x=x, z=z, blob=foreign_blob(kind, salt + k), label=f"set_columns: {kind} at ({x}, {z})"))
            for k, (kind, (x, z)) in enumerate(group_columns(at).items())]


def group_box(at, y0=0, y1=DIMS[1], margin=1):
    return (at[0] - margin, y0, at[1] - margin), (at[0] + 3 * SPACING + 1 + margin, y1, at[1] + 1 + margin)


def assert_foreign(solid, colour, at):
    """The group's columns hold what they are named for: y 0 .. 19 and 36 .. 45 solid, the runs of the split encodings touch, the shared colours
    are shared, the air column is empty."""
    cols = group_columns(at)
    for kind in FOREIGN:
        x, z = cols[kind]
        assert solid[x, 0:20, z].all() and solid[x, 36:46, z].all() and solid[x, :, z].sum() == 30, kind
    runs = FOREIGN["split solid run"][0]
    assert runs[1][0] != AIR and runs[2][0] != AIR and runs[4][0] != AIR and runs[5][0] != AIR, "two solid runs touch at y = 42 and at y = 8"
    assert sum(n for _, n in runs[:2]) == DIMS[1] - 42 and sum(n for _, n in runs[:5]) == DIMS[1] - 8
    runs = FOREIGN["split air run"][0]
    assert runs[0][0] == runs[1][0] == AIR and runs[3][0] == runs[4][0] == AIR and runs[0][1] == DIMS[1] - 54, "two air runs touch at y = 54 and at y = 27"
    x, z = cols["shared colours"]
    assert len({int(c) for c in colour[x, 36:46, z]} & {int(c) for c in colour[x, 0:20, z]}) == 10, "the shared colours are shared"
    x, z = cols["all air"]
    assert not solid[x, :, z].any() and all(ci == AIR for ci, _ in ALL_AIR[0]) and len(ALL_AIR[0]) > 1


# one group per call under test, away from each other and from the world's crater and slabs' edges: (x, z) of the group's first column
READER_GROUPS = {"read_heights": (10, 8), "distance": (40, 8), "surface": (70, 8), "spread": (100, 8), "nav": (10, 28), "report_cavities": (40, 28),
                 "read_voxels": (70, 28), "read_model": (100, 28)}
WRITER_GROUPS = {"write_voxels": (10, 68), "write_heights": (40, 68), "place_models": (70, 68), "copy": (100, 68), "stamp": (10, 88), "fill_cavities": (40, 88),
                 "lamps": (70, 88), "shapes": (100, 88)}


def _column(at, kind, box):
    """Index of the group's column `kind` in an (X, Z, ...) array over `box`."""
    x, z = group_columns(at)[kind]
    return x - box[0][0], z - box[0][2]


def _pocket(at):
    """Level-0 strokes, one call each, whose rectangles hold no foreign column: a block beside the split solid run's column with a tunnel of
    2 x 3 x 1 voxels that the column's upper run closes."""
    x, z = at
    return [_box(FILL, (x + 1, 35, z - 1), (x + 4, 42, z + 2), 0xFF707070), _box(CARVE, (x + 1, 37, z), (x + 3, 40, z + 1))]


def _has_pocket(m, want):
    return 6 in want[0]["voxels"].tolist()


def reader_plans():
    """{call: the steps behind the group's upload}; every box sits where the encoding matters (asserted by `holds` from the model)."""
    plans = {}
    at = READER_GROUPS["read_heights"]
    windows = {(0, 40): (40, 36), (0, 42): (42, 36), (0, 45): (45, 36), (0, 15): (15, 0), (40, 64): (46, 40), (8, 30): (20, 8), (0, 64): (46, 36)}
    plans["read_heights"] = []
    for (y0, y1), (height, bottom) in windows.items():  # the top inside the lower half, on the split, in the upper half; the bottom between the halves
        box = group_box(at, y0, y1)
        i = _column(at, "split solid run", box)
        plans["read_heights"].append(("read_heights", dict(box=box, label=f"read_heights, window [{y0}, {y1})",
                                                           holds=lambda m, want, i=i, h=height, b=bottom: want[0][i] == h and want[2][i] == b)))
    at = READER_GROUPS["distance"]
    box = group_box(at, margin=2)
    i = _column(at, "split solid run", box)
    # (columns of many runs stand within three columns of every place of this world: straight up or down is the nearest way only close by)
    plans["distance"] = [("distance", dict(box=box, mode=TO_SOLID, label="distance to solid",
                                           holds=lambda m, want, i=i: want[i][47] == 4 and want[i][46] == 1 and want[i][35] == 1 and want[i][20] == 1)),
                         ("distance", dict(box=box, mode=TO_AIR, label="distance to air",
                                           holds=lambda m, want, i=i: want[i][38] == 1 and want[i][41] == 1 and want[i][8] >= 1))]
    at = READER_GROUPS["surface"]
    box = group_box(at)
    x, z = group_columns(at)["split solid run"]
    sx, sz = group_columns(at)["shared colours"]

    def one_quad_per_side(m, want, x=x, z=z):
        q = want[0][(want[0]["voxel"][:, 0] == x) & (want[0]["voxel"][:, 2] == z) & (want[0]["voxel"][:, 1] == 36) & (want[0]["face"] != 2)]
        return len(q) == 4 and (q["length"] == 10).all()

    def shared(m, want, x=sx, z=sz):
        q = want[0][(want[0]["voxel"][:, 0] == x) & (want[0]["voxel"][:, 2] == z) & (want[0]["face"] == 0)]
        argb = {int(v[1]): int(c) for v, c in zip(q["voxel"], q["argb"])}  # (the k-th voxel of either run from its top has the k-th shared colour)
        low = [y for y in argb if y < 20]
        return len(low) >= 3 and all(argb[y] == argb[y + 26] for y in low) and len(set(argb.values())) == 10

    plans["surface"] = [("surface", dict(box=box, flags=IGNORE, label="surface, colours ignored", holds=one_quad_per_side)),
                        ("surface", dict(box=box, flags=0, label="surface with colours", holds=shared))]
    at = READER_GROUPS["spread"]
    x, z = group_columns(at)["split solid run"]
    ax, az = group_columns(at)["split air run"]
    plans["spread"] = []
    for y0 in (42 - 64, 8, 0):  # a 64-voxel chunk begins at the upper split, at the lower one, at neither
        box = group_box(at, y0, 64)
        i, a = _column(at, "split solid run", box), _column(at, "split air run", box)
        plans["spread"].append(("spread", dict(box=box, seeds=[(x, 45, z), (x, 19, z)], medium=SPREAD_SOLID, step_faces=UP_AND_DOWN, label=f"spread down the split run, box from y = {y0}",
                                               holds=lambda m, want, i=i, y0=y0: want[0][i][36 - y0] == 9 and (y0 > 0 or want[0][i][0 - y0] == 19))))
        plans["spread"].append(("spread", dict(box=box, seeds=[(ax, 63, az)], medium=SPREAD_AIR, step_faces=UP_AND_DOWN, label=f"spread through the split air run, box from y = {y0}",
                                               holds=lambda m, want, a=a, y0=y0: want[0][a][46 - y0] == 17)))
    at = READER_GROUPS["nav"]
    x, z = group_columns(at)["split solid run"]
    steps = [_box(FILL, (x + 1, 0, z), (x + 2, 45, z + 1), 0xFF909090), _box(FILL, (x - 1, 0, z), (x, 19, z + 1), 0xFF909090)]  # a step up onto either run
    plans["nav"] = [("brush", dict(strokes=[s], label=f"nav: step {k}", level_count=0)) for k, s in enumerate(steps)]
    plans["nav"].append(("nav", dict(call=(*group_box(at, margin=2), 1, 2, 1, 3, 0), goals=[(x, 46, z), (x, 20, z)], label="nav onto the split run",
                                     holds=lambda m, want, x=x, z=z: want[0][x, 46, z]["distance"] == 0 and want[0][x + 1, 45, z]["distance"] == 1
                                     and want[0][x, 20, z]["distance"] == 0 and want[0][x - 1, 19, z]["distance"] == 1)))
    at = READER_GROUPS["report_cavities"]
    plans["report_cavities"] = [("brush", dict(strokes=[s], label=f"pocket stroke {k}", level_count=0)) for k, s in enumerate(_pocket(at))]
    plans["report_cavities"].append(("report_cavities", dict(box=group_box(at, 30, 48, margin=2), label="cavities REPORT beside the split run", holds=_has_pocket)))
    at = READER_GROUPS["read_voxels"]
    box = group_box(at, margin=0)
    i = _column(at, "shared colours", box)

    def twice(m, want, i=i):
        values = np.unique(want[0][i][36:46])
        both = np.concatenate([want[0][i][36:46], want[0][i][0:20]])
        return len(values) == 10 and all(int((both == v).sum()) == 2 for v in values)

    plans["read_voxels"] = [("read_voxels", dict(box=box, label="read_voxels over the four columns", holds=twice))]
    at = READER_GROUPS["read_model"]
    lo, hi = group_box(at, margin=0)
    size = tuple(hi[k] - lo[k] for k in range(3))
    plans["read_model"] = [("read_model", dict(src_min=lo, size=size, transform=0, label="read_model over the four columns", holds=twice)),
                           ("read_model", dict(src_min=lo, size=size, transform=1, label="read_model over the four columns, a quarter turn"))]
    return plans


def writer_plans():
    """{call: the steps behind the group's upload}, everything at levelCount 0.  Every op leaves voxels of the foreign columns outside what it
    writes, so the re-emitted columns must merge the split runs and unshare the colours."""
    plans = {}
    at = WRITER_GROUPS["write_voxels"]
    lo, hi = group_box(at, 10, 16, margin=0)
    shape = (hi[0] - lo[0], hi[2] - lo[2], 6)
    plans["write_voxels"] = [("write_voxels", dict(write=(lo, _argb(shape, 41), None, FILL), label="dense FILL over y 10 .. 15", level_count=0))]
    at = WRITER_GROUPS["write_heights"]
    lo, hi = group_box(at, 0, 64, margin=1)
    shape = (hi[0] - lo[0], hi[2] - lo[2])
    plans["write_heights"] = [("write_heights", dict(write=(lo, 64, np.full(shape, 44, dtype=np.int32), _argb(shape, 43), _argb(shape, 44), 3, 0, PAINT),
                                                     label="heights PAINT, the crust y 41 .. 43", level_count=0))]
    at = WRITER_GROUPS["place_models"]
    instances = [identity_at((gx, 38, gz), (1, 6, 1), 0, CARVE) for gx, gz in group_columns(at).values()]
    plans["place_models"] = [("place_models", dict(models=[(None, np.ones((1, 1, 6), dtype=bool))], instances=instances, label="models CARVE, one voxel wide through y 38 .. 43",
                                                    level_count=0))]
    at = WRITER_GROUPS["copy"]
    lo, hi = group_box(at, 30, 50, margin=0)
    plans["copy"] = [("copy", dict(placements=[dict(srcMin=list(lo), srcMax=list(hi), dst=[lo[0], 22, lo[2]], transform=0, op=FILL, move=0)],
                                   label="copy: the foreign columns onto themselves, 8 lower", level_count=0))]
    at = WRITER_GROUPS["stamp"]
    lo, hi = group_box(at, margin=0)
    mesh = dict(position=[[lo[0], 30.5, lo[2]], [hi[0], 30.5, lo[2]], [lo[0], 30.5, hi[2]]], rgba=[[250, 10, 10, 255], [10, 250, 10, 255], [10, 10, 250, 255]], indices=[0, 1, 2])
    plans["stamp"] = [("stamp", dict(mesh=mesh, op=FILL, label="stamp FILL, one triangle at y = 30", level_count=0))]
    at = WRITER_GROUPS["fill_cavities"]
    plans["fill_cavities"] = [("brush", dict(strokes=[s], label=f"pocket stroke {k}", level_count=0)) for k, s in enumerate(_pocket(at))]
    # (levelCount 2: the pocket's own columns hold no foreign one, the rectangle rounded to 4 holds the split run's)
    plans["fill_cavities"].append(("fill_cavities", dict(box=group_box(at, 30, 48, margin=2), label="cavities FILL of the pocket", level_count=2)))
    at = WRITER_GROUPS["lamps"]
    box = group_box(at, 30, 64, margin=1)  # (the lower runs lie below the box)
    plans["lamps"] = [("lamps", dict(p=_sun(box, sky_range=3), lamps=[lampmodel.lamp((at[0] + 2, 50, at[1]), 10, 255), lampmodel.lamp((at[0] + 6, 28, at[1] + 1), 9, 200)],
                                     label="lamps over the foreign columns", level_count=0))]
    at = WRITER_GROUPS["shapes"]
    lo, hi = group_box(at, margin=0)
    plans["shapes"] = [("shapes", dict(strokes=[_capsule(PAINT, (lo[0], 40, lo[2]), (hi[0] - 1, 38, lo[2]), 2, 0xFF3366CC)], label="capsule PAINT through the upper runs", level_count=0))]
    return plans


# ---- D. partial refreshes by newer writers ----------------------------------------------------------------------------------------------------------

_D_SHELL = _shell(8, 51)
_D_HEIGHTS = _hills((8, 4, 8), (16, 16), 4, 40, 53)
PARTIAL_SETUP = ("write_voxels", dict(write=((100, 24, 100), *_shell(8, 52), REPLACE), label="a shell for the cavities FILL, every level refreshed"))  # before the case begins
PARTIAL = [
    ("write_heights", dict(write=((8, 4, 8), 40, *_D_HEIGHTS, 2, 0, REPLACE), label="heights write, levelCount 2", level_count=2)),
    ("place_models", dict(models=[(_argb((3, 3, 5), 3), None), (None, np.ones((2, 2, 9), dtype=bool))], instances=_chain((40, 14, 40), 70, (FILL,)),
                          label="models place, levelCount 2", level_count=2)),
    ("write_voxels", dict(write=((12, 24, 72), _D_SHELL[0], _D_SHELL[1], REPLACE), label="dense write, levelCount 2", level_count=2)),
    ("fill_cavities", dict(box=((96, 20, 96), (112, 36, 112)), label="cavities FILL, levelCount 2", level_count=2)),
]
PARTIAL_RECTS = [(8, 8, 16, 16), (40, 40, 48, 25), (12, 72, 8, 8), (101, 101, 6, 6)]  # the four footprints at levelCount 0, rounded to 4 below
PARTIAL_STAMP = ("stamp", dict(mesh=_quad((2, 26, 2), (60, 36, 60), 5), op=FILL, label="stamp, levelCount 5", level_count=5))
PARTIAL_READS = [
    ("distance", dict(box=((8, 0, 8), (24, 48, 24)), mode=SIGNED, label="distance over the heights write")),
    ("distance", dict(box=((40, 0, 40), (56, 48, 56)), mode=TO_SOLID, label="distance over the models place")),
    ("spread", dict(box=((8, 0, 68), (24, 64, 84)), seeds=[(9, 60, 69)], medium=SPREAD_AIR, label="spread around the dense write's shell")),
    ("spread", dict(box=((96, 0, 96), (112, 64, 112)), seeds=[(104, 27, 104)], medium=SPREAD_SOLID, label="spread through the filled shell")),
    ("spread", dict(box=((6, 0, 6), (90, 64, 66)), seeds=[(7, 60, 7)], medium=SPREAD_AIR, label="spread over the first two rectangles")),
]
PARTIAL_LAMPS = ("lamps", dict(p=_sun(((0, 0, 0), DIMS), sky_range=3, sun_range=32), lamps=[lampmodel.lamp((16, 44, 16), 12, 255), lampmodel.lamp((44, 40, 44), 16, 230),
                                                                                             lampmodel.lamp((16, 40, 76), 12, 200)], label="lamps over the whole world"))


def rounded(rect, level):
    k = (1 << level) - 1
    x0, z0 = rect[0] & ~k, rect[1] & ~k
    x1, z1 = min((rect[0] + rect[2] + k) & ~k, DIMS[0]), min((rect[1] + rect[3] + k) & ~k, DIMS[2])
    return x0, z0, x1 - x0, z1 - z0


def refreshed(columns, level):
    """The rectangle a writer that changed `columns` (bool[dimX, dimZ]) refreshes at levelCount `level`, where its footprint is what it changed."""
    xs, zs = np.nonzero(columns)
    return rounded((int(xs.min()), int(zs.min()), int(xs.max() - xs.min()) + 1, int(zs.max() - zs.min()) + 1), level)


def _overlap(a, b):
    return a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]


# ---- the tests: every plan on the models alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sparse", [False, True])
def test_the_editors_loop_is_valid_on_the_models(work, sparse):
    run = ModelRun(DIMS, *sequence_world(31, sparse), work)
    run.run(LOOP_SETUP + LOOP_FIRST)
    run.run(LOOP_SECOND)
    writers = [c for c, _ in LOOP_FIRST if c in WRITERS]
    assert writers == ["stamp", "copy", "write_heights", "place_models", "write_voxels", "fill_cavities", "lamps", "shapes"] == [c for c, _ in LOOP_SECOND if c in WRITERS]
    assert all(a.get("overlaps") for c, a in LOOP_FIRST[1:] + LOOP_SECOND if c in WRITERS), "every writer overlaps the one before it"


def test_the_tall_loop_crosses_the_steps_on_edited_columns(work):
    run = ModelRun(TALL, *tall_world(), work)
    run.run(tall_loop(0))
    crossing = [(x, z) for x in range(TALL[0]) for z in range(TALL[2]) if run.last[x, z] and any(run.solid[x, s - 1, z] and run.solid[x, s, z] for s in (64, 128, 192))]
    assert crossing, "a column the last writer changed holds a run across a 64-voxel step"
    run.run(tall_loop(1))


@pytest.mark.parametrize("writer", sorted(BEHIND_A_COMPACTION))
def test_the_writers_behind_a_compaction_change_the_edited_columns(work, writer):
    run = ModelRun(DIMS, *sequence_world(80, False), work)
    moved = np.zeros((DIMS[0], DIMS[2]), dtype=bool)
    for step in strokes_plan(SETUP, "setup stroke"):
        run.run([step])
        moved |= run.last
    for call, args in BEHIND_A_COMPACTION[writer]:
        if call == "compact":
            continue
        run.run([(call, args)])
        if call in WRITERS and "behind the compaction" in args["label"]:
            assert (run.last & moved).any(), f"{args['label']} changes a column that a setup stroke moved"


def test_the_terrain_exceeds_the_tails_headroom(work):
    """What can be said from the volumes: the write needs more colour slots than cvx_edit.hip's headroom rule leaves behind an edit of a world
    whose every column held `depth` colours at the most (the GPU test asserts the same need against the spare bytes the context reports)."""
    run = ModelRun(DIMS, *sequence_world(90, False), work)
    run.run(strokes_plan(SETUP, "setup stroke"))
    old = run.solid
    edited = (old != sequence_world(90, False)[0]).any(axis=1)
    run.run(RELAYOUT[:1])
    need = relayout_need(old, run.solid, edited)
    assert need > 2 * headroom(slots_in_use(old)), (need, headroom(slots_in_use(old)))
    run.run(RELAYOUT[1:])


def test_the_foreign_groups_hold_what_they_are_named_for(work):
    for groups, plans in ((READER_GROUPS, reader_plans()), (WRITER_GROUPS, writer_plans())):
        run = ModelRun(DIMS, *sequence_world(100, False), work)
        assert set(groups) == set(plans)
        for salt, at in enumerate(groups.values()):
            run.run(group_plan(at, 10 * salt))
            assert_foreign(run.solid, run.colour, at)
        taken = np.zeros((DIMS[0], DIMS[2]), dtype=bool)
        for at in groups.values():
            for x, z in group_columns(at).values():
                taken[x, z] = True
        for call, plan in plans.items():
            before = run.solid.copy(), run.colour.copy()
            for name, args in plan:
                run.run([(name, args)])
                if name == "brush":  # the rectangle of a levelCount-0 brush beside a group holds none of its columns
                    assert not (run.last & taken).any(), args["label"]
            if groups is WRITER_GROUPS:  # the writer changes its own group and leaves voxels of it outside what it writes; the others stay
                mine = np.zeros_like(taken)
                for x, z in group_columns(groups[call]).values():
                    mine[x, z] = True
                assert (_columns(refreshed(run.last, plan[-1][1]["level_count"]), DIMS) & mine).any(), f"{call}: the writer re-emits no foreign column"
                assert not (_columns(refreshed(run.last, plan[-1][1]["level_count"]), DIMS) & taken & ~mine).any(), f"{call}: the writer re-emits another group's column"
                diff = (run.solid != before[0]) | (run.colour != before[1])
                for kind, (x, z) in group_columns(groups[call]).items():
                    assert kind == "all air" or (run.solid[x, :, z] & ~diff[x, :, z]).sum() >= 10, f"{call}: {kind} keeps voxels the writer left alone"
                assert not diff.any(axis=1)[taken & ~mine].any(), f"{call}: the other groups stay as they were uploaded"


def test_the_partial_refreshes_overlap_as_the_case_says(work):
    run = ModelRun(DIMS, *sequence_world(61, False), work)
    run.run([PARTIAL_SETUP])
    for (call, args), rect in zip(PARTIAL, PARTIAL_RECTS):
        run.run([(call, args)])
        xs, zs = np.nonzero(run.last)
        assert rect[0] <= xs.min() and xs.max() < rect[0] + rect[2] and rect[1] <= zs.min() and zs.max() < rect[1] + rect[3], (args["label"], xs.min(), xs.max(), zs.min(), zs.max())
    assert not any(_overlap(rounded(a, 2), rounded(b, 2)) for k, a in enumerate(PARTIAL_RECTS) for b in PARTIAL_RECTS[k + 1:]), "four separate rectangles"
    run.run([PARTIAL_STAMP])
    stamp = refreshed(run.last, 5)
    hit = [_overlap(stamp, rounded(r, 2)) for r in PARTIAL_RECTS]
    assert hit == [True, True, False, False], f"the stamp's rounded rectangle {stamp} overlaps two of the four"
    run.run(PARTIAL_READS + [PARTIAL_LAMPS])
