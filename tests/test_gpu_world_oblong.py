"""GPU: the world calls and repeat mode on worlds that are not square -- LONG_Z = 32 x 64 x 256 (rowShift 8, dimX 32) and LONG_X = 256 x 64 x 32
(rowShift 5, dimX 256) of tests/oblongworlds.py.  (x << rowShift) + z, the clips against dimX / dimZ, the wraps with maskX / maskZ and the
rounding of edit rectangles all read the same on the wrong axis in the square worlds of the other GPU tests.

The call lists are those of tests/oblongworlds.py, which tests/test_oblong_worlds_cpu.py runs on the models alone and asserts there that every case
reaches past the short side; here _Oblong, a _Later of tests/test_gpu_world_sequences_later.py, runs the same lists on a context beside the models.
Every comparison is bytes or integers against the dense model the call's own test file uses.  Behind a writer LOD 0 .. levelCount are compared with
the host-built chain of the model's world and the levels above with the world before the call; behind a reader every level and edit_stats() are as
before.  Every size comes LONG_Z first: a swapped axis stays inside the record table there and shows as a failed comparison."""
import numpy as np
import pytest

import oblongworlds as ob
import oraclelib as O
import pickmodel
import piecesmodel
import repeatworld as R
import scenes
from cpuvox_amd import gpu
from oblongworlds import SIZES
from test_gpu_world_brush import _brushed, _hits
from test_gpu_world_copy import _assert_levels
from test_gpu_world_edit import _check_world
from test_gpu_world_edit import _context as _render_context
from test_gpu_world_edit import _frames as _bounded_frames
from test_gpu_world_move import _assert_all_routes
from test_gpu_world_pieces import _report as _pieces_report
from test_gpu_world_repeat import CLEAR, H, POSES, W, _draw, _mismatch, _same
from test_gpu_world_repeat import _context as _repeat_context
from test_gpu_world_sequences_later import _Later
from test_gpu_world_snapshot import _diff_against_model, held, voxels
from test_gpu_world_surface_rects import _rects
from test_world_light_cpu import model_world
from test_world_move_cpu import bodies_to_array, model_results, world_bodies
from test_world_sequences_later_cpu import work  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WRITER_NAMES = list(ob.writer_cases(ob.LONG_Z))
READER_NAMES = list(ob.reader_cases(ob.LONG_Z))
WORLDS = [(dims, sparse) for sparse in (False, True) for dims in SIZES]


@pytest.fixture(scope="module")
def uploads():
    """{(dims, sparse): (solid, colour, WorldSet, a context of it that nothing writes into)}: one upload per size and world."""
    out = {}
    for dims, sparse in WORLDS:
        solid, colour, ws = (ob.sparse_world if sparse else ob.dense_world)(dims)
        ctx = gpu.Context(0)
        ctx.upload_world(ws)
        ctx.read_level(0)  # (places the levels in the arena: edit_stats() counts them from here on)
        solid.setflags(write=False)
        colour.setflags(write=False)
        out[dims, sparse] = (solid, colour, ws, ctx)
    yield out
    for _, _, ws, ctx in out.values():
        ctx.close()
        ws.close()


def _levels(ctx):
    return [ctx.read_level(k) for k in range(6)]


class _Oblong(_Later, ob.OblongModels):
    """_Later on an oblong world.  ctx: the shared context of the readers; without it a fresh one (a writer's).

    Which parent supplies what (the MRO is _Oblong, _Later, _Sequence, OblongModels, Models):
    - _Later: the device calls of the newer writers and readers (stamp, copy, write_heights, ..., read_model), apply() and unchanged();
    - _Sequence: the device calls brush, light, settle, compact and check(); its remove() is replaced here by one that takes a levelCount;
    - OblongModels: the models m_light, m_settle, m_remove, m_edit, m_snapshot_restore (its own: snapshot, strokes and restore in one step, which
      replaces the named snapshots of _Later / Models here), m_lift_remove, m_lift_copy and the readers' m_* that record where a result reaches,
      and changed(); Models below it: the other m_* that _Later's calls use;
    - here: run(), world(), the device calls remove, edit, set_columns, snapshot_restore, surface_rects and report_pieces.
    No parent constructor runs, as in _LaterTall: _Sequence's builds the square world and OblongModels' knows no context, so the state of both
    (steps, work, last, before, default; written, seen) is set here."""
    quick = True

    def __init__(self, dims, upload, work, ctx=None):
        self.dims = dims
        self.solid, self.colour, self.ws, shared = upload
        self.owns = ctx is None
        self.ctx = ctx
        if self.owns:
            self.ctx = gpu.Context(0)
            self.ctx.upload_world(self.ws)
        self.steps, self.work, self.last, self.before, self.default = 0, work, None, None, None
        self.written = np.zeros((dims[0], dims[2]), dtype=bool)
        self.seen = np.zeros((dims[0], dims[2]), dtype=bool)

    def close(self):
        if self.owns:
            self.ctx.close()

    def world(self):
        return model_world(self.dims, self.solid, self.colour)

    def run(self, plan):
        """A writer below levelCount 5 refreshes LOD 0 .. levelCount: the levels above stay the world's before it."""
        for call, args in plan:
            level_count = args.get("level_count", 5)
            old = self.world() if level_count < 5 else None
            try:
                if old is not None:
                    self.default = lambda label, old=old, level_count=level_count: self.check_up_to(old, level_count, label)
                getattr(self, call)(**args)
            finally:
                self.default = None
                if old is not None:
                    old.close()

    def check_up_to(self, old, level_count, label):
        new = self.world()
        try:
            _assert_levels(self.ctx, new, old, level_count, f"step {self.steps} ({label})")
        finally:
            new.close()

    # -- the writers the newer sequences do not run ---------------------------------------------------------------------------------------------------
    def remove(self, box, anchors, label, level_count=5):
        want, want_summary, _ = piecesmodel.analyse(self.solid, *box, anchors)
        pieces, summary, _ = self.ctx.world_pieces(*box, anchors, gpu.PIECES_REMOVE, level_count=level_count, capacity=8192)
        assert summary == want_summary and pieces.tobytes() == want[:8192].tobytes(), label
        self.apply(piecesmodel.remove(self.solid, self.colour, *box, anchors), label)

    def edit(self, rect, strokes, label, level_count=5):
        after = self.m_edit(rect, strokes, label)
        want = model_world(self.dims, *after)
        try:
            blob, count = want.extract_region(0, *rect)
        finally:
            want.close()
        assert self.ctx.edit(*rect, blob, count, level_count) > 0.0
        self.apply(after, label)

    def set_columns(self, rect, strokes, label):
        """cvx_world_set_columns on each level in turn: after level l LOD 0 .. l are the edited world's, the rest as they were."""
        after = self.m_edit(rect, strokes, label)
        want, old = model_world(self.dims, *after), self.world()
        try:
            for lod in range(6):
                r = [v >> lod for v in rect]
                blob, count = want.extract_region(lod, *r)
                self.ctx.set_columns(lod, *r, blob, count)
                _assert_levels(self.ctx, want, old, lod, f"{label}, after level {lod}")
        finally:
            want.close()
            old.close()
        self.apply(after, label)

    def snapshot_restore(self, rect, strokes, label, level_count=5):
        self.m_snapshot_restore(rect, strokes, label)
        before = _levels(self.ctx)
        with self.ctx.world_snapshot(*rect, level_count) as snapshot:
            assert held(snapshot) == ob.rounded(rect, level_count, self.dims), label
            self.ctx.brush(strokes, level_count)
            assert self.ctx.read_level(0) != before[0], f"{label}: the strokes change nothing"
            assert snapshot.restore() > 0.0
        assert _levels(self.ctx) == before, f"{label}: the world is not as it was when the snapshot was taken"
        self.steps += 1
        self.check(label)

    # -- and the readers -----------------------------------------------------------------------------------------------------------------------------
    def surface_rects(self, box, label, solid_outside=0x04, flags=0, holds=None):
        stats = self.ctx.edit_stats()
        _rects(self.ctx, self.solid, self.colour, *box, solid_outside, flags, label=label)
        self.unchanged(stats, label)

    def report_pieces(self, box, anchors, label, holds=None):
        stats = self.ctx.edit_stats()
        pieces, _ = _pieces_report(self.ctx, self.solid, *box, anchors, capacity=8192, label=label)
        assert len(pieces) > 0, label
        self.unchanged(stats, label)


# ---- the writers --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("name", WRITER_NAMES)
def test_a_writer(uploads, work, dims, name):
    for plan in ob.writer_cases(dims)[name]:
        s = _Oblong(dims, uploads[dims, False], work)
        try:
            s.run(plan)
        finally:
            s.close()


@pytest.mark.parametrize("dims", SIZES)
def test_a_copy_whose_source_would_fit_if_the_axes_were_swapped_is_rejected(uploads, dims):
    ws = uploads[dims, False][2]
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        with pytest.raises(gpu.CvxError, match="outside the world"):
            ctx.copy([ob.copy_rejected(dims)], 5)
        assert ctx.edit_stats()[1:] == (0, 0)
        assert _levels(ctx) == [(ws.storage(k).tobytes(), ws.info(k).columnCount) for k in range(6)]
    finally:
        ctx.close()


# ---- the readers ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("name", READER_NAMES)
def test_a_reader(uploads, work, dims, name):
    fresh = name in ob.NEEDS_SHELLS
    s = _Oblong(dims, uploads[dims, False], work, None if fresh else uploads[dims, False][3])
    try:
        s.run(ob.reader_cases(dims)[name])
        assert fresh or not s.written.any()
    finally:
        s.close()


@pytest.mark.parametrize("dims,sparse", WORLDS)
def test_read_back_is_byte_identical(uploads, dims, sparse):
    """read_level, read_region (the whole level, a rectangle up to the far corner, random ones) and download against the upload's own blobs."""
    _, _, ws, ctx = uploads[dims, sparse]
    rng = np.random.default_rng(11)
    stats = ctx.edit_stats()
    for k in range(6):
        assert ctx.read_level(k) == (ws.storage(k).tobytes(), ws.info(k).columnCount), f"LOD {k}"
        used_x, used_z = dims[0] >> k, dims[2] >> k
        rects = [(0, 0, used_x, used_z), (used_x // 2 + (k < 4), used_z // 2 + (k < 3), used_x - used_x // 2 - (k < 4), used_z - used_z // 2 - (k < 3))]
        for _ in range(6):
            sx, sz = int(rng.integers(1, used_x + 1)), int(rng.integers(1, used_z + 1))
            rects.append((int(rng.integers(0, used_x - sx + 1)), int(rng.integers(0, used_z - sz + 1)), sx, sz))
        for rect in rects:
            assert ctx.read_region(k, *rect) == ws.extract_region(k, *rect), f"LOD {k} rectangle {rect}"
    saved = ctx.download()
    try:
        for k in range(6):
            assert saved.storage(k).tobytes() == ws.storage(k).tobytes() and saved.info(k).columnCount == ws.info(k).columnCount, f"download, LOD {k}"
    finally:
        saved.close()
    assert ctx.edit_stats() == stats


@pytest.mark.parametrize("dims", SIZES)
@pytest.mark.parametrize("repeat", [False, True])
def test_moves(uploads, dims, repeat):
    solid, _, ws, _ = uploads[dims, False]
    bodies = world_bodies(ob.SEED, solid, repeat, 1000) + ob.seam_bodies(dims)
    want = model_results(solid, bodies, repeat)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        ctx.set_world_repeat(repeat)
        before, stats = _levels(ctx), ctx.edit_stats()
        _assert_all_routes(ctx, bodies_to_array(bodies), want, f"{dims} repeat {repeat}")
        assert _levels(ctx) == before and ctx.edit_stats() == stats
    finally:
        ctx.close()


@pytest.mark.parametrize("dims", SIZES)
def test_picks_bounded_and_repeating(uploads, dims):
    solid, colour, ws, _ = uploads[dims, False]
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        before, stats = _levels(ctx), ctx.edit_stats()
        o, d, max_t = pickmodel.random_rays(np.random.default_rng(5), dims, 2000)
        so, sd, side = ob.seam_rays(dims)
        o, d, max_t = np.concatenate([o, so]), np.concatenate([d, sd]), np.concatenate([max_t, np.full(len(so), ob.SEAM_MAX_T, np.float32)])
        got = _hits(ctx.pick(o, d, max_t))
        model = pickmodel.pick_many(solid, colour, o, d, max_t)
        fraction = pickmodel.compare_picks(got, model, f"{dims} bounded")
        assert fraction >= 0.99, f"only {fraction:.4f} of the rays are unambiguous"
        hit = got["face"] >= 0
        assert (got["argb"][hit] == colour[tuple(got["voxel"][hit].T)]).all(), "the hit colour is the voxel's"
        # repeating: the rays leave through each of the four sides and re-enter; the bounded model walks the world laid out around them
        ctx.set_world_repeat(True)
        t_solid, t_colour, at = ob.tiled(dims, solid, colour)
        got = _hits(ctx.pick(so + at, sd, ob.SEAM_MAX_T))
        vox, face, argb, t, amb = pickmodel.pick_many(t_solid, t_colour, so + at, sd, ob.SEAM_MAX_T)
        wrapped = np.where((face >= 0)[:, None], vox % np.array([dims[0], 1 << 30, dims[2]]), vox).astype(np.int32)
        fraction = pickmodel.compare_picks(got, (wrapped, face, argb, t, amb), f"{dims} repeating")
        assert fraction >= 0.99, f"only {fraction:.4f} of the rays are unambiguous"
        for s in range(4):
            tiles = (vox[(face >= 0) & (side == s)][:, [0, 2]] // np.array([dims[0], dims[2]])) != (at[[0, 2]] // np.array([dims[0], dims[2]])).astype(np.int64)
            assert tiles.any(axis=1).sum() >= 3, f"rays through side {s} re-enter and hit"
        assert _levels(ctx) == before and ctx.edit_stats() == stats
    finally:
        ctx.close()


# ---- snapshots and the arena ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims,sparse", WORLDS)
def test_snapshot_diff_and_diff_device(uploads, dims, sparse):
    """Snapshots of the whole footprint, of a rectangle up to the far corner and of one that overhangs all four sides; forty strokes along the long
    axis; every diff is the model's (both flags, prefixes, the device list) and changes nothing."""
    ws = uploads[dims, sparse][2]
    strokes = ob.tower_strokes(dims, 40)
    ctx = gpu.Context(0)
    try:
        ctx.upload_world(ws)
        before = voxels(ctx, dims)
        snapshots = [ctx.world_snapshot(*ob.rect_of(box), level_count) for box, level_count in ((ob.whole(dims), 5), (ob.corner(dims), 0), (ob.corner(dims), 2), (ob.overhang(dims), 5))]
        for stroke in strokes:
            ctx.brush([stroke], 5)
        levels, stats = _levels(ctx), ctx.edit_stats()
        for k, snapshot in enumerate(snapshots):
            counts = _diff_against_model(ctx, snapshot, before, f"{dims} snapshot {k}")
            assert counts[0] > 0, f"snapshot {k}: nothing changed inside it"
        assert _levels(ctx) == levels and ctx.edit_stats() == stats
        for snapshot in snapshots:
            snapshot.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("dims,sparse", WORLDS)
def test_compaction_and_relayout_under_a_snapshot(uploads, work, dims, sparse):
    """A snapshot of the whole world; forty one-stroke brushes along the long axis; a compaction that leaves every level as before it; a terrain over
    the whole footprint that does not fit the tails, so that the arena is laid out again; the snapshot restored."""
    s = _Oblong(dims, uploads[dims, sparse], work)
    strokes = ob.tower_strokes(dims, 40)
    try:
        start = _levels(s.ctx)
        snapshot = s.ctx.world_snapshot(0, 0, dims[0], dims[2], 5)
        for stroke in strokes:
            s.ctx.brush([stroke], 5)
        s.apply(_brushed(s.solid, s.colour, strokes), "forty strokes")
        used, abandoned, spare = s.ctx.edit_stats()
        assert abandoned > 0, "block moves leave their old places behind"
        before = _levels(s.ctx)
        reclaimed, ms = s.ctx.compact()
        used2, abandoned2, spare2 = s.ctx.edit_stats()
        assert abandoned2 == 0 and reclaimed == used - used2 and reclaimed > 0 and ms > 0.0, (used, abandoned, used2, reclaimed)
        assert _levels(s.ctx) == before, "the compaction changed a level"
        assert s.ctx.compact()[0] == 0
        s.write_heights(ob.relayout_write(dims), "a terrain over the whole footprint")
        used3, _, spare3 = s.ctx.edit_stats()
        assert used3 + spare3 > used2 + spare2, "the arena has not been laid out again (used + spare: no edit inside the tails changes it)"
        assert spare3 >= 4 * 16384, (used3, spare3)
        assert snapshot.restore() > 0.0
        assert _levels(s.ctx) == start, "the snapshot restored behind the compaction and the relayout"
        snapshot.close()
    finally:
        s.close()


# ---- rendering --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", SIZES)
def test_a_bounded_frame_after_a_brush_is_the_rebuilds(uploads, dims):
    """Both kernels draw the brushed world as the CPU oracle and a fresh upload of the host rebuild do."""
    solid, colour, ws, _ = uploads[dims, False]
    strokes = [s for plan in ob.writer_cases(dims)["brush"] for _, args in plan for s in args["strokes"] if s["shape"] in (gpu.SHAPE_BOX, gpu.SHAPE_SPHERE)]
    want = model_world(dims, *_brushed(solid, colour, strokes))
    ctx = _render_context(ws)
    try:
        ctx.brush(strokes, 5)
        _check_world(ctx, want, _bounded_frames(want)[1:3], f"{dims} brushed")
    finally:
        ctx.close()
        want.close()


REPEAT_WORLDS = {"stripes32x64x128": (64, 16), "proc128x64x32": (16, 64)}  # name -> the tile counts that make T 2048 x 2048 columns
FAR_CLIP = 400.0  # (the reference's 10 x the largest dimension does not fit the short axis)


def _repeat_frames(ws, tiles):
    centre = [tiles[a] * ws.dims[2 * a] / 2.0 for a in range(2)]
    room = [c - FAR_CLIP - 33.0 for c in centre]  # (the far clip plus one LOD-5 cell from T's edge, per axis)
    assert min(room) > 0
    out = []
    for (ox, oz), fy, eul, err in POSES:
        fr = R.frame(ws, W, H, (centre[0] + ox * room[0], fy * ws.dims[1], centre[1] + oz * room[1]), eul, FAR_CLIP, err)
        assert fr.camera.FarClip + 32 <= centre[0] - abs(ox) * room[0] and fr.camera.FarClip + 32 <= centre[1] - abs(oz) * room[1], "the camera is too close to T's edge"
        out.append(fr)
    return out


@pytest.mark.parametrize("name", list(REPEAT_WORLDS))
def test_repeat_render_equals_the_tiled_bounded_world(name):
    """W repeated renders exactly as the bounded T = W laid out to 2048 x 2048 columns, through both kernels; T is the CPU oracle's in two poses."""
    ws = scenes.load_world(name)
    tiles = REPEAT_WORLDS[name]
    assert ws.dims[0] != ws.dims[2] and (tiles[0] * ws.dims[0], tiles[1] * ws.dims[2]) == (2048, 2048)
    wt = R.tile_world(ws, *tiles)
    frames = _repeat_frames(ws, tiles)
    cw, ct = _repeat_context(ws, True), _repeat_context(wt, None)
    try:
        for i, fr in enumerate(frames):
            for mode, kernel in ((gpu.LATENCY_ALWAYS, "latency"), (gpu.LATENCY_NEVER, "batch")):
                _same(f"{name} pose {i} {kernel} kernel", _draw(cw, fr, mode), _draw(ct, fr, mode))
        for i in (0, 4):
            o_td, o_lr, _ = O.draw_segments(wt, frames[i], W, H, clear=CLEAR, counters=False)
            n_td, n_lr = scenes.used_rows(frames[i])
            _same(f"{name}: T pose {i} vs oracle", _draw(ct, frames[i], gpu.LATENCY_NEVER), (o_td[:n_td], o_lr[:n_lr]))
        cb = _repeat_context(ws, None)  # the same world drawn bounded differs: the comparison above went through the repeat path
        try:
            assert any(_mismatch(_draw(cb, fr, gpu.LATENCY_NEVER), _draw(cw, fr, gpu.LATENCY_NEVER)) > 0 for fr in frames)
        finally:
            cb.close()
    finally:
        cw.close()
        ct.close()
        wt.close()
