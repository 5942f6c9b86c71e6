"""-m gpu: Phase 2 (blit_kernel, blit_batch_kernel, and blit_classify inside the image gather; cvx_kernels.h) over the blit catalogue
(tests/blitposes.py): partial tiles both ways, screens smaller than a tile and wider than 2048, seams through pixel centres, the vanishing point
at the screen centre and far off screen, one-segment frames, a repeating world.

The raybuffers are drawn by the batch kernel and by the latency kernel.  Every image is compared bit for bit with the numpy statement of the rule
(oraclelib.blit_reference) over the GPU's own raybuffers AND over the CPU oracle's, so the picture a caller sees -- not only Phase 1 -- is pinned to
the oracle; tests/test_blit_rule_cpu.py checks that numpy rule against an independent float64 one.  Nothing here launches out of range: a store past
a partial tile would land in the next row, the next image or a guard area of the caller's buffer, all of which are compared."""
import numpy as np
import pytest

import blitposes as B
import edgeposes as E
import oraclelib as O
import repeatworld as R
from cpuvox_amd import gpu

pytestmark = pytest.mark.gpu

CLEAR = B.RAY_CLEAR
BOTH_KERNELS = [("batch kernel", gpu.LATENCY_NEVER), ("latency kernel", gpu.LATENCY_ALWAYS)]
GUARD = 0x5A5A5A5A
UNWRITTEN = 0x77777777
NAMES = [b.name for b in sorted(B.CATALOGUE, key=lambda b: (b.world, b.width, b.height))]  # (one world after the other, a resolution at a time)


class _Contexts:
    """One context per world (and per emulated rank of the image gather), its resolution and buffer count set per use."""

    def __init__(self):
        self.cache = {}

    def get(self, world, W, H, buffers=2, rank=None):
        key = (world, rank)
        if key not in self.cache:
            ctx = gpu.Context(0)
            ctx.upload_world(E.load_world(world))
            self.cache[key] = ctx
        ctx = self.cache[key]
        if ctx.buffer_count != buffers:
            ctx.set_buffer_count(buffers)
        ctx.set_resolution(W, H)
        return ctx

    def close(self):
        for ctx in self.cache.values():
            ctx.close()


@pytest.fixture(scope="module")
def contexts():
    c = _Contexts()
    yield c
    c.close()


_oracle = {}


def _oracle_raybuffers(b):
    """The CPU oracle's raybuffers of an entry (cleared to the sentinel), rendered once per session."""
    if b.name not in _oracle:
        ws, fr = B.frame(b)
        td, lr, _ = O.draw_segments(ws, fr, b.width, b.height, clear=CLEAR, counters=False)
        _oracle[b.name] = (fr, td, lr)
    return _oracle[b.name]


def _render_gpu(ctx, fr, latency, buffer=0):
    ctx.set_latency_kernel(latency)
    try:
        ctx.clear_raybuffers(buffer, CLEAR)
        ctx.draw_segments(fr, buffer)
    finally:
        ctx.set_latency_kernel(gpu.LATENCY_AUTO)
    return ctx.read_raybuffer(buffer, gpu.RAYBUFFER_TOPDOWN), ctx.read_raybuffer(buffer, gpu.RAYBUFFER_LEFTRIGHT)


def _differ(label, got, want):
    d = got != want
    if d.any():
        ys, xs = np.nonzero(d)
        raise AssertionError(f"{label}: {int(d.sum())} of {d.size} screen pixels differ; first at x {xs[0]} y {ys[0]}: got {got[ys[0], xs[0]]:08x} "
                             f"want {want[ys[0], xs[0]]:08x}; columns {xs.min()}..{xs.max()}, rows {ys.min()}..{ys.max()}")


@pytest.mark.parametrize("name", NAMES)
def test_single_blit_bit_exact(contexts, name):
    """cvx_blit_segments == the numpy rule over the GPU's own raybuffers and over the oracle's, for both render kernels; no pixel of the image is an
    unwritten raybuffer pixel; away from every boundary the image is the float64 rule's."""
    b = B.BY_NAME[name]
    W, H = b.width, b.height
    fr, o_td, o_lr = _oracle_raybuffers(b)
    want = O.blit_reference(fr, o_td, o_lr, W, H, clear=0)
    ref64, margin = O.blit_reference_f64(fr, o_td, o_lr, W, H, clear=0)
    ctx = contexts.get(b.world, W, H)
    for label, mode in BOTH_KERNELS:
        g_td, g_lr = _render_gpu(ctx, fr, mode)
        img = ctx.blit_segments(0)
        assert img.shape == (H, W)
        _differ(f"{name} [{label}] against the rule over the GPU's raybuffers", img, O.blit_reference(fr, g_td, g_lr, W, H, clear=0))
        _differ(f"{name} [{label}] against the rule over the oracle's raybuffers", img, want)
        assert not (img == CLEAR).any(), f"{name} [{label}]: {(img == CLEAR).sum()} image pixels are raybuffer pixels nothing wrote"
        differ = img != ref64
        assert not (differ & (margin > 1e-4)).any(), f"{name} [{label}]: {(differ & (margin > 1e-4)).sum()} pixels away from every boundary differ from the float64 rule"
        if "vp_centre" not in b.tags and "tiny" not in b.tags:  # (tests/test_blit_rule_cpu.py: where the share says nothing)
            assert differ.mean() < 2e-3, f"{name} [{label}]: {differ.sum()} pixels differ from the float64 rule"


def test_blit_matches_pixel_centre_rule(contexts):
    for name in ("scene_mill256_t075", "scene_mill256_t09_roll", "scene_proc256_t0_lod8"):
        b = B.BY_NAME[name]
        W, H = b.width, b.height
        ws, fr = B.frame(b)
        ctx = contexts.get(b.world, W, H)
        for label, mode in BOTH_KERNELS:
            g_td, g_lr = _render_gpu(ctx, fr, mode)
            img = ctx.blit_segments(0)
            ref = O.blit_reference(fr, g_td, g_lr, W, H, clear=0)
            assert (img == ref).all(), f"{name} [{label}]: {(img != ref).sum()} screen pixels differ"
            # ... and an independent check (float64 barycentrics, none of the kernel's edge-function arithmetic): the images may differ only where a
            # weight or a ray coordinate lies within rounding distance of a boundary, and those pixels are a sliver of the screen
            ref64, margin = O.blit_reference_f64(fr, g_td, g_lr, W, H, clear=0)
            differ = img != ref64
            assert not (differ & (margin > 1e-4)).any(), f"{name} [{label}]: {(differ & (margin > 1e-4)).sum()} pixels away from every boundary differ from the float64 rule"
            assert differ.mean() < 2e-3, f"{name} [{label}]: {differ.sum()} pixels differ from the float64 rule"


def test_batch_blit_equals_single_blits():
    """cvx_blit_segments_batch (Phase 2 of a whole batch in one launch, images left on the device) == cvx_blit_segments frame by frame,
    both into a caller's device buffer (a torch tensor) and into the array the context owns."""
    import torch

    names = ["scene_proc256_t0_lod8", "scene_proc256_t04_lod8", "scene_proc256_t075_lod8", "scene_proc256_t075_lod1"]  # one world, one resolution
    frames = []
    for n in names:
        b = B.BY_NAME[n]
        ws, fr = B.frame(b)
        W, H = b.width, b.height
        frames.append(fr)
    ctx = gpu.Context(0, buffer_count=len(frames) + 1)
    try:
        ctx.upload_world(ws)
        ctx.set_resolution(W, H)
        for b in range(len(frames) + 1):
            ctx.clear_raybuffers(b, 0)
        ctx.draw_segments_batch(frames, 1)  # buffers 1 .. n
        singles = [ctx.blit_segments(1 + i) for i in range(len(frames))]
        dst = torch.zeros((len(frames), H, W), dtype=torch.int32, device="cuda:0")
        p = ctx.blit_segments_batch(1, len(frames), dst.data_ptr())
        assert p == dst.data_ptr()
        ctx.synchronize()
        got = dst.cpu().numpy().view(np.uint32)
        for i, n in enumerate(names):
            assert (got[i] == singles[i]).all(), f"{n}: batch blit differs from the single blit in {(got[i] != singles[i]).sum()} pixels"
            td = ctx.read_raybuffer(1 + i, gpu.RAYBUFFER_TOPDOWN)
            lr = ctx.read_raybuffer(1 + i, gpu.RAYBUFFER_LEFTRIGHT)
            assert (got[i] == O.blit_reference(frames[i], td, lr, W, H, clear=0)).all(), n
        # context-owned image array: same pixels (read back through a torch view of the returned address is not possible, so blit a
        # sub-range twice and compare the two device arrays on the device)
        own = ctx.blit_segments_batch(2, 2)
        assert own and own != dst.data_ptr()
        with pytest.raises(RuntimeError):
            ctx.blit_segments_batch(1, len(frames) + 1)  # past the last buffer
        with pytest.raises(RuntimeError):
            ctx.blit_segments_batch(0, 1)                # buffer 0 was never drawn into
    finally:
        ctx.close()


def _groups(entries):
    g = {}
    for b in entries:
        g.setdefault((b.world, b.width, b.height), []).append(b)
    return g


@pytest.mark.parametrize("key", sorted(_groups(B.CATALOGUE)), ids=lambda k: f"{k[0]}_{k[1]}x{k[2]}")
def test_batch_blit_by_resolution(contexts, key):
    """The batch blit (64 rows per workgroup) of every catalogue frame, one launch per world and resolution with as many buffers as the group has
    frames, into a caller's torch buffer: each image == the single blit == the rule over the oracle's raybuffers.  The buffer has a guard area of a
    sentinel before and after the images (at least one image row each) and starts out as a second sentinel: every pixel must have been stored,
    none outside."""
    import torch

    world, W, H = key
    entries = _groups(B.CATALOGUE)[key]
    n = len(entries)
    frames = [_oracle_raybuffers(b)[0] for b in entries]
    ctx = contexts.get(world, W, H, buffers=n)
    guard = max(W, 4096)
    for label, mode in BOTH_KERNELS:
        ctx.set_latency_kernel(mode)
        try:
            for i in range(n):
                ctx.clear_raybuffers(i, CLEAR)
            ctx.draw_segments_batch(frames, 0)
        finally:
            ctx.set_latency_kernel(gpu.LATENCY_AUTO)
        singles = [ctx.blit_segments(i) for i in range(n)]
        buf = torch.full((guard + n * H * W + guard,), GUARD, dtype=torch.int32, device="cuda:0")
        buf[guard:guard + n * H * W] = UNWRITTEN
        torch.cuda.synchronize()
        p = ctx.blit_segments_batch(0, n, buf.data_ptr() + 4 * guard)
        assert p == buf.data_ptr() + 4 * guard
        ctx.synchronize()
        flat = buf.cpu().numpy().view(np.uint32)
        assert (flat[:guard] == GUARD).all() and (flat[guard + n * H * W:] == GUARD).all(), f"{key} [{label}]: the batch blit stored outside its images"
        got = flat[guard:guard + n * H * W].reshape(n, H, W)
        for i, b in enumerate(entries):
            fr, o_td, o_lr = _oracle_raybuffers(b)
            _differ(f"{b.name} [{label}] batch blit against the single blit", got[i], singles[i])
            _differ(f"{b.name} [{label}] batch blit against the rule over the oracle's raybuffers", got[i], O.blit_reference(fr, o_td, o_lr, W, H, clear=0))


GATHER_TAGS = ("partial_width", "seam_through_centres", "tiny")
GATHER_GROUPS = _groups([b for b in B.CATALOGUE if any(t in b.tags for t in GATHER_TAGS)])


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("key", sorted(GATHER_GROUPS), ids=lambda k: f"{k[0]}_{k[1]}x{k[2]}")
def test_image_gather_of_partial_seam_and_tiny_frames(contexts, key, N):
    """The image gather (cvx_image_plan_*, pack, unpack; ranks emulated on one GPU as in test_image_gather_emulated_on_one_gpu) of the frames tagged
    partial_width, seam_through_centres or tiny, a launch per world and resolution: the display rank's image == the single blit (which
    test_single_blit_bit_exact pins to the oracle); every pixel travels at most once."""
    import torch

    world, W, H = key
    entries = GATHER_GROUPS[key]
    frames = [_oracle_raybuffers(b)[0] for b in entries]
    dev = torch.device("cuda", 0)
    whole = contexts.get(world, W, H)
    expected = []
    for fr in frames:
        _render_gpu(whole, fr, gpu.LATENCY_NEVER)
        expected.append(whole.blit_segments(0))
    ranks = []
    try:
        for r in range(N):
            ctx = contexts.get(world, W, H, rank=r)
            packed = ctx.pack_batch(frames)
            plan = gpu.ImagePlan(ctx, packed, W, H, r, N)
            store = torch.zeros(max(1, plan.local_store_bytes // 4), dtype=torch.int32, device=dev)
            send = torch.full((max(1, plan.send_pixels),), 0x55, dtype=torch.int32, device=dev)
            recv = torch.full((max(1, plan.recv_pixels),), 0x66, dtype=torch.int32, device=dev)
            images = torch.full((max(1, plan.images), H, W), 0x77, dtype=torch.int32, device=dev)
            ranks.append((ctx, plan, send, recv, images))
            ctx.draw_placed(packed, plan.tile_out(store.data_ptr()))
            plan.pack(ctx, None, store.data_ptr(), send.data_ptr(), images.data_ptr())
            ctx.synchronize()
        assert sum(p.images for _, p, _, _, _ in ranks) == len(frames)
        for r, (_, plan, send, _, _) in enumerate(ranks):
            for q, (_, qplan, _, qrecv, _) in enumerate(ranks):
                s0, sn, _, _ = plan.transfer(q)
                _, _, r0, rn = qplan.transfer(r)
                assert sn == rn and (q != r or sn == 0)
                assert s0 + sn <= max(1, plan.send_pixels) and r0 + rn <= max(1, qplan.recv_pixels)
                if sn:
                    qrecv[r0:r0 + rn].copy_(send[s0:s0 + sn])
        torch.cuda.synchronize()
        total_sent = sum(p.send_pixels for _, p, _, _, _ in ranks)
        assert total_sent <= len(frames) * W * H, (total_sent, len(frames), W, H)
        for r, (ctx, plan, _, recv, images) in enumerate(ranks):
            plan.unpack(ctx, None, recv.data_ptr(), images.data_ptr())
            ctx.synchronize()
            got = images.cpu().numpy().view(np.uint32)
            for i, b in enumerate(entries):
                if i % N == r:
                    _differ(f"image gather: {b.name} on rank {r} of {N}", got[i // N], expected[i])
    finally:
        for _, plan, _, _, _ in ranks:
            plan.close()


def test_repeating_world_blit():
    """One frame of a repeating world (cvx_set_world_repeat) at an odd size with roll: its blit == the blit of the same world laid out 16 x 16 times
    == the rule over the oracle's raybuffers of the tiled world."""
    k, far, W, H = 16, 300.0, 97, 65
    ws = E.load_world("terrace64")
    wt = R.tile_world(ws, k)
    c = k * ws.dims[0] // 2
    pos = (c + 20.0, 16.0, c + 20.0)
    assert far + 32 <= min(pos[0], pos[2], k * ws.dims[0] - pos[0], k * ws.dims[2] - pos[2])
    fr = R.frame(ws, W, H, pos, (10.0, 90.0, 30.0), far)
    o_td, o_lr, _ = O.draw_segments(wt, fr, W, H, clear=CLEAR, counters=False)
    want = O.blit_reference(fr, o_td, o_lr, W, H, clear=0)
    assert sum(1 for s in fr.segments if s.RayCount > 0) >= 2 and not (want == CLEAR).any()
    cw, ct = gpu.Context(0), gpu.Context(0)
    try:
        cw.upload_world(ws)
        ct.upload_world(wt)
        cw.set_resolution(W, H)
        ct.set_resolution(W, H)
        cw.set_world_repeat(True)
        for label, mode in BOTH_KERNELS:
            _render_gpu(ct, fr, mode)
            tiled = ct.blit_segments(0)
            _render_gpu(cw, fr, mode)
            _differ(f"repeating world [{label}] against the tiled world", cw.blit_segments(0), tiled)
            _differ(f"tiled world [{label}] against the rule over the oracle's raybuffers", tiled, want)
    finally:
        cw.close()
        ct.close()
