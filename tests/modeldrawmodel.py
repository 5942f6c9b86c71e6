"""An independent numpy model of cvxv_models_draw (include/cpuvox_gpu_model_draw.h): the rays of a view from numpy's own float64 arithmetic, the
bodies through tests/modelpickmodel.py, the world through tests/pickmodel.py (picked to the far limit and compared with the body's t, not cut at
it).  It shares no code with cpuvox_amd/csrc/cvx_model_draw.h and calls a pixel AMBIGUOUS where a rule with other rounding may answer
differently: the body pick says so, the world pick says so, or the world's hit and the body's lie within EPS of each other."""
import numpy as np

import modelpickmodel
import pickmodel

EPS = 1e-4


def view_rays(view):
    """(origins float32 (h, w, 3), directions float32 (h, w, 3), good bool (h, w)) of a gpu.DrawView, row 0 the bottom row."""
    w, h = view.width, view.height
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    a = np.array(view.dir0[:])[None, None, :] + x[..., None] * np.array(view.dirX[:]) + y[..., None] * np.array(view.dirY[:])
    length = np.linalg.norm(a, axis=-1)
    good = (length > 0) & np.isfinite(length)
    d = np.where(good[..., None], a / np.where(good, length, 1.0)[..., None], 0.0).astype(np.float32)
    return np.broadcast_to(np.array(view.origin[:], dtype=np.float32), d.shape).copy(), d, good


def draw(models, instances, view, flags=0, world=None, image=None, depth=None, ids=None, draw_world=1, depth_test=2):
    """-> (image uint32 (h, w), depth float64 (h, w), ids int32 (h, w), ambiguous bool (h, w), {pixelsDrawn, pixelsOccluded}).  `instances` as
    dicts (tests/test_world_models_cpu.as_dicts), `world` a (solid, colour) pair of (x, y, z) volumes; the arrays given are copied."""
    w, h = view.width, view.height
    image = np.zeros((h, w), dtype=np.uint32) if image is None else np.array(image, dtype=np.uint32)
    out_depth = np.full((h, w), np.inf) if depth is None else np.array(depth, dtype=np.float64)
    ids = np.full((h, w), -1, dtype=np.int32) if ids is None else np.array(ids, dtype=np.int32)
    o, d, good = view_rays(view)
    limit = np.full((h, w), np.float32(view.maxT), dtype=np.float32)
    amb = np.zeros((h, w), dtype=bool)
    if flags & depth_test:
        held = np.asarray(depth, dtype=np.float32)
        good = good & (held >= 0)
        limit = np.where(held < limit, held, limit)
    hits, hit_amb = modelpickmodel.pick_many(models, instances, o.reshape(-1, 3), d.reshape(-1, 3), np.where(good, limit, np.float32(-1)).ravel())
    hits, amb = hits.reshape(h, w), amb | hit_amb.reshape(h, w)
    drawn = occluded = 0
    for y in range(h):
        for x in range(w):
            hit = hits[y, x]
            if hit["instance"] < 0:
                continue
            shows = True
            if flags & draw_world:
                _, face, _, t_world, world_amb = pickmodel.pick(world[0], world[1], o[y, x], d[y, x], limit[y, x])
                amb[y, x] |= world_amb
                if face >= 0:
                    shows = t_world > hit["t"]
                    amb[y, x] |= abs(t_world - hit["t"]) < EPS
            if shows:
                drawn += 1
                image[y, x], out_depth[y, x], ids[y, x] = hit["argb"], hit["t"], hit["instance"]
            else:
                occluded += 1
    return image, out_depth, ids, amb, {"pixelsDrawn": drawn, "pixelsOccluded": occluded}


def compare(got, model, label):
    """(image, depth, ids) of a call against draw()'s output: exact image and ids, depth within pickmodel.compare_picks' tolerance, on the
    unambiguous pixels.  -> the unambiguous fraction."""
    image, depth, ids = got
    want_image, want_depth, want_ids, amb, _ = model
    ok = ~amb
    close = np.isclose(np.asarray(depth, dtype=np.float64), want_depth, rtol=1e-5, atol=1e-5) | (np.asarray(depth, dtype=np.float64) == want_depth)
    bad = ok & ((image != want_image) | (ids != want_ids) | ~close)
    if bad.any():
        y, x = [int(v[0]) for v in np.nonzero(bad)]
        raise AssertionError(f"{label}: {int(bad.sum())} of {int(ok.sum())} unambiguous pixels differ; first ({x}, {y}): got id {ids[y, x]} depth {depth[y, x]} "
                             f"argb {image[y, x]:08x}, want id {want_ids[y, x]} depth {want_depth[y, x]} argb {want_image[y, x]:08x}")
    return float(ok.mean())
